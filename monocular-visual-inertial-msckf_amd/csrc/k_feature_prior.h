// K1-K4 of a track whose point carries a prior (msckf_set_point_priors; point_prior.h): 1 to FEATP_MAXM (= MSCKF_MAX_TRACK_PRIOR)
// views, one workgroup of four wavefronts per track, launched over the list of the batch's prior tracks only.  The plain
// kernels (k_feature, k_feature_wide) skip those tracks by the byte they skip unselected tracks by (FeatureArgs::select is
// pointed at k_prior_prepare's mask for their launches) and are otherwise what they were.
//
//   K1  per-view residual and Jacobians           reference MSCKF.py:505-544, Camera.py:54-67   (view_row.h)
//       + three prior rows [sigma W | 0 | sigma W (pbar - p_lin)]                                (point_prior.h)
//   K2  left-nullspace projection of the (2M + 3) x 3 block   reference MSCKF.py:554-559
//   K3  chi-square gate against the prior P, 2M degrees of freedom   reference MSCKF.py:561-568
//   K4  the block [H_o | r_o], 2M x (6M + 1), row-major at blk_off[f]   reference MSCKF.py:581-588
//
// Row layout: thread t < 2M owns measurement row t (view t >> 1, image axis t & 1), threads 2M .. 2M + 2 the prior rows, whose
// row of D is zero.  The three column-pivoted Householder reflectors run over all 2M + 3 rows (first wavefront, one row per
// lane: 2M + 3 <= 63); H_o = D - V Z with Z = T^T (V^T D) as in k_feature, rows 3 .. 2M + 2.  The gate and the elimination
// are k_feature_wide's (E = H_o P_sub and S = E H_o^T + sigma^2 I on the fp64 matrix cores, a strip of 16 rows per wavefront:
// q = 2M <= 60 rows are at most one strip each), on q = 2M rows.
//
// The verdict's `rank` is what K5's row count 2M - rank needs (FeatureArgs::rank): 0.  A block whose rank test finds fewer than
// three pivots (a prior so loose that sigma W vanishes beside H_f) would leave more than 2M rows: verdict 0, nothing written.
//
// Linearise at the mean (MSCKF_PRIOR_AT_MEAN): k_prior_prepare writes the run's m', rho' into arrays of the run's own, which
// every K1 of the run -- this kernel, k_robust, the plain kernels (whose tracks' entries are copies) -- reads in place of the
// batch's; the batch's are only read.
//
// No wait on another workgroup, no atomics, every loop bounded by M.  fp64 only (the host refuses priors on an f32 context).
#pragma once
#include <hip/hip_runtime.h>
#include "wave_ops.h"
#include "k_feature.h"            // FeatureArgs, feature_verdict, view_row.h
#include "k_feature_wide.h"       // FEATW_ET_LD, wave_sync
#include "point_prior.h"

namespace msckf {

constexpr int FEATP_T = 256;      // threads of a workgroup: one per row (2M + 3 <= 63) in K1, four wavefronts in the gate
constexpr int FEATP_MAXM = kMaxTrackPrior;
constexpr int FEATP_ROWS = 64;    // rows the carve-up holds: 2 FEATP_MAXM + 3, rounded up

struct PriorPrepareArgs {
    int F;                        // tracks, sorted order
    const unsigned char* has;     // [F] 1: the track carries a prior
    const unsigned char* select;  // optional [F] flags of k_select
    unsigned char* mask;          // [F] out: what the plain kernels take as `select` -- bit 0 off for a prior track
    int at_mean;                  // MSCKF_PRIOR_AT_MEAN: fill m_out / rho_out
    const double* mean;           // [3F]
    const double* base;           // [3F]
    const double* m_in;           // [3F] the batch's points (read only)
    const double* rho_in;         // [F]
    double* m_out;                // [3F] the run's points: m', rho' for a prior track, a copy for the others
    double* rho_out;              // [F]
};

__global__ __launch_bounds__(256) void k_prior_prepare(PriorPrepareArgs p) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= p.F) return;
    const bool has = p.has[f] != 0;
    p.mask[f] = has ? (unsigned char)0 : (p.select ? p.select[f] : (unsigned char)1);
    if (!p.at_mean) return;
    double m[3] = {p.m_in[3 * f], p.m_in[3 * f + 1], p.m_in[3 * f + 2]}, rho = p.rho_in[f];
    if (has) (void)point_prior_at_mean(p.mean + 3 * f, p.base + 3 * f, m, &rho);     // (false: the track keeps its own point)
    p.m_out[3 * f] = m[0]; p.m_out[3 * f + 1] = m[1]; p.m_out[3 * f + 2] = m[2];
    p.rho_out[f] = rho;
}

struct FeaturePriorArgs {
    FeatureArgs a;                // as k_feature takes them (split, f0 unused); select: the run's own flags, not the mask
    const int* list;              // [gridDim.x] sorted indices of the batch's prior tracks: workgroup b takes track list[b]
    const double* W;              // [9F] the whitening L^-1 of the track's prior (sorted order; read for listed tracks)
    const double* mean;           // [3F] pbar
    double sigma;
    double* d2;                   // [F] out: (pbar - p_lin)^T Sigma_p^-1 (pbar - p_lin) at the run's linearisation point
};

// LDS carve-up (doubles), sized for FEATP_MAXM views whatever the track holds: 33.2 KiB, four workgroups per CU
struct FeatPriorLayout {
    static constexpr int V = FEATP_MAXM, R = FEATP_ROWS;
    static constexpr int slot = 0;                        // int [V]
    static constexpr int A = slot + (V + 1) / 2 + 1;      // [R][6]  OC-projected clone block rows (D); zero for the prior rows
    static constexpr int Vr = A + R * 6;                  // [R][3]  H_f | sigma W rows (K1), then the Householder vectors' rows
    static constexpr int res = Vr + R * 3;                // [R]     r
    static constexpr int ro = res + R;                    // [R]     r_o = Q^T r
    static constexpr int Z = ro + R;                      // [3][6V]
    static constexpr int misc = Z + 3 * 6 * V;            // T (6 doubles), rank (int at [8])
    static constexpr int Et = misc + 16;                  // [4][16][17] a wavefront's tile of E
    static constexpr int S = Et + 4 * 16 * FEATW_ET_LD;   // packed lower triangle of [S ; r_o^T]: (2V + 1)(2V + 2) / 2
    static constexpr int total = S + (2 * V + 1) * (2 * V + 2) / 2;
};
static_assert(2 * FEATP_MAXM + 3 <= FEATP_ROWS && FEATP_ROWS <= 64, "k_feature_prior: K2 holds one row per lane");
static_assert((size_t)FeatPriorLayout::total * 8 <= 48 * 1024, "k_feature_prior: LDS of one workgroup");

__global__ __launch_bounds__(FEATP_T) void k_feature_prior(FeaturePriorArgs w) {
    typedef double v4d_ __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) double smem[FeatPriorLayout::total];
    const FeatureArgs& p = w.a;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int f = w.list[blockIdx.x];
    const int v0 = p.view_ptr[f];
    const int M = p.view_ptr[f + 1] - v0;
    if (M < 1 || M > FEATP_MAXM) {            // (never sent by the host: nothing below may index past the carve-up)
        if (t == 0) { feature_verdict(p, f, 0, 0.0, 0); w.d2[f] = 0.0; }
        return;
    }
    const int R2 = 2 * M, C6 = 6 * M, RA = R2 + 3;      // RA: rows of the augmented block
    int* sSlot = reinterpret_cast<int*>(smem + FeatPriorLayout::slot);
    double* sA = smem + FeatPriorLayout::A;
    double* sV = smem + FeatPriorLayout::Vr;
    double* sRes = smem + FeatPriorLayout::res;
    double* sRo = smem + FeatPriorLayout::ro;
    double* sZ = smem + FeatPriorLayout::Z;
    double* sMisc = smem + FeatPriorLayout::misc;
    double* sEt = smem + FeatPriorLayout::Et + wv * 16 * FEATW_ET_LD;
    double* sS = smem + FeatPriorLayout::S;

    if (p.select && !(p.select[f] & 1)) {      // not in valid_features (MSCKF.py:453-455): no rows, not a rejection
        if (t == 0) { feature_verdict(p, f, 0, 0.0, 3); w.d2[f] = 0.0; }
        return;
    }
    // ---------------- K1: one row per thread: 2M measurement rows (view_row.h), three prior rows (point_prior.h) ------------
    if (t < R2) {
        const int view = t >> 1;
        const int o = v0 + view;
        const int s = p.obs_slot[o];
        if ((t & 1) == 0) sSlot[view] = s;
        const double* R = p.cam_R + 9 * s;
        const double* tt = p.cam_t + 3 * s;
        const ViewPoint vp = view_point(R, tt, p.idp_base + 3 * f, p.idp_m + 3 * f, p.idp_rho[f], p.Kinv, p.obs_uv[2 * o], p.obs_uv[2 * o + 1]);
        const ViewRow vr = view_row(vp, R, tt, p.cam_R0 + 9 * s, p.cam_t0 + 3 * s, p.g, t & 1, p.obs_w ? p.obs_w + o : nullptr);
#pragma unroll
        for (int a = 0; a < 6; ++a) sA[t * 6 + a] = vr.a[a];
        sV[t * 3 + 0] = vr.h[0]; sV[t * 3 + 1] = vr.h[1]; sV[t * 3 + 2] = vr.h[2];
        sRes[t] = vr.res;
    } else if (t < RA) {
        double pl[3];
        point_prior_lin(p.idp_base + 3 * f, p.idp_m + 3 * f, p.idp_rho[f], pl);
        const PriorRow pr = point_prior_row(w.W + 9 * (size_t)f, w.mean + 3 * (size_t)f, pl, w.sigma, t - R2);
#pragma unroll
        for (int a = 0; a < 6; ++a) sA[t * 6 + a] = 0.0;
        sV[t * 3 + 0] = pr.h[0]; sV[t * 3 + 1] = pr.h[1]; sV[t * 3 + 2] = pr.h[2];
        sRes[t] = pr.res;
        if (t == R2) w.d2[f] = point_prior_distance(w.W + 9 * (size_t)f, w.mean + 3 * (size_t)f, pl);
    }
    __syncthreads();
    // ---------------- K2: column-pivoted Householder QR of [H_f ; sigma W], the first wavefront with row `lane` per lane --------
    // After step k row k holds R_kk; rows >= 3 span the left null space.  The rank decision is k_feature's.
    if (wv == 0) {
        const bool in = lane < RA;
        double c0 = in ? sV[lane * 3 + 0] : 0.0, c1 = in ? sV[lane * 3 + 1] : 0.0, c2 = in ? sV[lane * 3 + 2] : 0.0;
        const double rs = in ? sRes[lane] : 0.0;
        double vv0 = 0, vv1 = 0, vv2 = 0;
        double beta0 = 0, beta1 = 0, beta2 = 0;
        int rank = 0;
        double r00 = 0.0;
        const double tol_scale = 2.220446049250313e-16 * (double)RA;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool act = in && lane >= k;
            double n0 = wave_sum(act ? c0 * c0 : 0.0);
            double n1 = (k < 2) ? wave_sum(act ? c1 * c1 : 0.0) : -1.0;
            double n2 = (k < 1) ? wave_sum(act ? c2 * c2 : 0.0) : -1.0;
            // pivot: bring the largest remaining column to the front (c0)
            if (n1 > n0 && n1 >= n2) { const double t_ = c0; c0 = c1; c1 = t_; n0 = n1; }
            else if (n2 > n0 && n2 > n1) { const double t_ = c0; c0 = c2; c2 = t_; n0 = n2; }
            const double ry = fast_rsqrt(n0);
            const double nrm = n0 * ry;
            if (k == 0) r00 = nrm;
            if (!(nrm > tol_scale * r00) || nrm == 0.0) break;   // numerically rank deficient (a zero column gives NaN and leaves here)
            const double xk = lane_bcast(c0, k);
            const double alpha = (xk > 0.0) ? -nrm : nrm;
            const double vk = act ? ((lane == k) ? (xk - alpha) : c0) : 0.0;
            const double beta = ry * fast_rcp(nrm + fabs(xk));   // 1 / (nrm (nrm + |xk|))
            if (k < 2) {
                const double d1 = wave_sum(vk * (act ? c1 : 0.0));
                if (act) c1 -= beta * d1 * vk;
            }
            if (k < 1) {
                const double d2 = wave_sum(vk * (act ? c2 : 0.0));
                if (act) c2 -= beta * d2 * vk;
            }
            if (k == 0) { vv0 = vk; beta0 = beta; }
            else if (k == 1) { vv1 = vk; beta1 = beta; }
            else { vv2 = vk; beta2 = beta; }
            rank = k + 1;
            c0 = c1; c1 = c2; c2 = 0.0;
        }
        // T of the compact WY form Q = I - V T V^T (forward, columnwise)
        const double v01 = wave_sum(vv0 * vv1), v02 = wave_sum(vv0 * vv2), v12 = wave_sum(vv1 * vv2);
        const double T00 = beta0, T11 = beta1, T22 = beta2;
        const double T01 = -beta1 * T00 * v01;
        const double T02 = -beta2 * (T00 * v02 + T01 * v12);
        const double T12 = -beta2 * T11 * v12;
        // residual: r_o = r - V T^T V^T r
        const double wr0 = wave_sum(vv0 * rs), wr1 = wave_sum(vv1 * rs), wr2 = wave_sum(vv2 * rs);
        const double zr0 = T00 * wr0;
        const double zr1 = T01 * wr0 + T11 * wr1;
        const double zr2 = T02 * wr0 + T12 * wr1 + T22 * wr2;
        if (in) {
            sV[lane * 3 + 0] = vv0; sV[lane * 3 + 1] = vv1; sV[lane * 3 + 2] = vv2;
            sRo[lane] = rs - (vv0 * zr0 + vv1 * zr1 + vv2 * zr2);
        }
        if (lane == 0) {
            sMisc[0] = T00; sMisc[1] = T01; sMisc[2] = T02; sMisc[3] = T11; sMisc[4] = T12; sMisc[5] = T22;
            reinterpret_cast<int*>(sMisc + 8)[0] = rank;
        }
    }
    __syncthreads();
    const int rank = reinterpret_cast<const int*>(sMisc + 8)[0];
    if (rank < 3) {                            // q would exceed the block's 2M rows: not stacked, a rejection (uniform)
        if (t == 0) feature_verdict(p, f, 0, 0.0, 0);
        return;
    }
    const int q = R2;                          // RA - 3
    // W = V^T D (a view's two rows; the prior rows of D are zero), Z = T^T W: one column of the 6M per thread and trip
    {
        const double T00 = sMisc[0], T01 = sMisc[1], T02 = sMisc[2], T11 = sMisc[3], T12 = sMisc[4], T22 = sMisc[5];
        for (int c = t; c < C6; c += FEATP_T) {
            const int vw = c / 6, a = c - 6 * vw;
            const double d0 = sA[(2 * vw) * 6 + a], d1 = sA[(2 * vw + 1) * 6 + a];
            const double* ve = sV + (2 * vw) * 3;
            const double w0 = ve[0] * d0 + ve[3] * d1, w1 = ve[1] * d0 + ve[4] * d1, w2 = ve[2] * d0 + ve[5] * d1;
            sZ[c] = T00 * w0;
            sZ[C6 + c] = T01 * w0 + T11 * w1;
            sZ[2 * C6 + c] = T02 * w0 + T12 * w1 + T22 * w2;
        }
    }
    __syncthreads();
    // ---------------- K4: rows 3 .. 2M + 2 of [H_o | r_o] = [D - V Z | r_o], contiguous in the stack block (2M rows) ------------
    const int ldb = C6 + 1;
    double* blk = static_cast<double*>(p.stack) + p.blk_off[f];
    {
        const int nel = q * ldb;
        for (int e = t; e < nel; e += FEATP_T) {
            const int L = e / ldb, cc = e - L * ldb;
            const int row = 3 + L;             // < RA
            double x;
            if (cc == C6) x = sRo[row];
            else {
                x = 0.0;
                x -= sV[row * 3 + 0] * sZ[cc];
                x -= sV[row * 3 + 1] * sZ[C6 + cc];
                x -= sV[row * 3 + 2] * sZ[2 * C6 + cc];
                const int vw = cc / 6;
                if (vw == (row >> 1)) x += sA[row * 6 + (cc - 6 * vw)];      // D: only the rows of the column's own view (never a prior row: row >> 1 >= M there)
            }
            blk[e] = x;
        }
        // [S ; r_o^T]: the extra row of the elimination
        for (int j = t; j < q; j += FEATP_T) sS[q * (q + 1) / 2 + j] = sRo[3 + j];
    }
    __threadfence_block();
    __syncthreads();                         // the gate reads the block this workgroup wrote
    // ---------------- K3: S = H_o P_sub H_o^T + sigma^2 I, lower triangle, a strip of 16 rows per wavefront (k_feature_wide's) -----
    {
        const int NI = (q + 15) >> 4, NC = (C6 + 15) >> 4;      // NI <= 4
        const int l15 = lane & 15, g4 = lane >> 4;
        constexpr int TRIP = 16;             // product steps of 4 whose loads are issued together
        for (int I = wv; I < NI; I += FEATP_T / 64) {
            v4d_ accS[4];
#pragma unroll
            for (int J = 0; J < 4; ++J) accS[J] = v4d_{0.0, 0.0, 0.0, 0.0};
            const int arow = 16 * I + l15;
            const bool aok = arow < q;
            const double* ap = blk + (size_t)(aok ? arow : 0) * ldb;
            for (int cc = 0; cc < NC; ++cc) {
                // the chunk's tile of E = H_o[strip, :] P_sub[:, chunk]
                const int bcol = 16 * cc + l15;
                const bool bok = bcol < C6;
                const int bc = bok ? bcol : 0;
                const double* bp = p.P + 15 + 6 * sSlot[bc / 6] + (bc % 6);
                v4d_ e = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < C6; k0 += 4 * TRIP) {
                    double av[TRIP], bv[TRIP];
#pragma unroll
                    for (int u = 0; u < TRIP; ++u) {
                        const int k = k0 + 4 * u + g4;
                        const bool kok = k < C6;
                        const int kc = kok ? k : 0;
                        const int kv = kc / 6;
                        av[u] = (aok && kok) ? ap[kc] : 0.0;
                        bv[u] = (bok && kok) ? bp[(size_t)(15 + 6 * sSlot[kv] + (kc - 6 * kv)) * p.ldp] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < TRIP; ++u) e = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], e, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) sEt[(g4 + 4 * r) * FEATW_ET_LD + l15] = e[r];
                wave_sync();                 // (a wavefront's LDS instructions execute in program order)
                // ... times H_o[strip J, chunk]^T into the strip's tiles of S, J <= I
                double ea[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) ea[kk] = sEt[l15 * FEATW_ET_LD + 4 * kk + g4];
#pragma unroll
                for (int J = 0; J < 4; ++J) {
                    if (J <= I) {
                        const int brow = 16 * J + l15;
                        const bool rok = brow < q;
                        const double* hp = blk + (size_t)(rok ? brow : 0) * ldb + 16 * cc + g4;
                        double hb[4];
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) hb[kk] = (rok && 16 * cc + 4 * kk + g4 < C6) ? hp[4 * kk] : 0.0;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) accS[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(ea[kk], hb[kk], accS[J], 0, 0, 0);
                    }
                }
                wave_sync();                 // the next chunk rewrites the tile
            }
#pragma unroll
            for (int J = 0; J < 4; ++J) {
                if (J <= I) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * I + g4 + 4 * r, j = 16 * J + l15;
                        if (i < q && j <= i) sS[i * (i + 1) / 2 + j] = accS[J][r] + (i == j ? p.sigma2 : 0.0);
                    }
                }
            }
        }
    }
    // ---------------- elimination of [S ; r_o^T] in LDS, all threads; column k is left unscaled (L_ik L_kk) -----------------------
    int bad = 0;
    {
        const int ty = t >> 4, tx = t & 15;
        for (int k = 0; k < q; ++k) {
            __syncthreads();                 // step k - 1 (k = 0: the strips of S) is complete
            const double piv = sS[k * (k + 1) / 2 + k];
            if (!(piv > 0.0)) { bad = 1; break; }      // (every thread reads the same word: uniform)
            const double rp = 1.0 / piv;
            for (int i = k + 1 + ty; i <= q; i += 16) {
                double* si = sS + i * (i + 1) / 2;
                const double lik = si[k] * rp;
                const int jmax = i < q ? i : q - 1;
                for (int j = k + 1 + tx; j <= jmax; j += 16) si[j] -= lik * sS[j * (j + 1) / 2 + k];
            }
        }
    }
    __syncthreads();
    if (wv == 0) {
        double gam = 0.0;
        if (!bad) {
            double part = 0.0;
            for (int k = lane; k < q; k += 64) { const double y = sS[q * (q + 1) / 2 + k]; part += y * y / sS[k * (k + 1) / 2 + k]; }
            gam = wave_sum(part);
        }
        bool ok = (bad == 0) && (q < p.n_chi2);
        if (ok) ok = (gam <= p.chi2[q]);
        // 1 accepted, 0 rejected by the gate, 2 the gate matrix was not SPD; rank 0: the block holds 2M - 0 rows
        if (lane == 0) feature_verdict(p, f, 0, gam, ok ? 1 : (bad ? 2 : 0));
    }
}

}  // namespace msckf
