// K1-K4 of a WIDE track: 32 to FEATW_MAXM (= MSCKF_MAX_TRACK_WIDE) views, one workgroup of four wavefronts per track.
//
//   K1  per-view residual and Jacobians           reference MSCKF.py:505-544, Camera.py:54-67
//   K2  left-nullspace projection of the H_f block reference MSCKF.py:554-559
//   K3  chi-square gate against the prior P        reference MSCKF.py:561-568
//   K4  the block [H_o | r_o], q x (6M + 1), row-major at blk_off[f]   reference MSCKF.py:581-588
//
// k_feature.h holds one measurement row per LANE, so 2M + 1 rows must fit one wavefront: 31 views.  Here a row belongs to a
// THREAD of the workgroup (K1: view_row.h, the text k_feature calls), the three column-pivoted Householder reflectors of H_f (2M x 3)
// are formed by the first wavefront with two rows per lane (K2), and H_o = D - V Z with Z = T^T (V^T D) (3 x 6M; k_feature.h's sZ) is
// written to the stack by all threads (K4).  At 64 views the block is 125 x 385 doubles: it lives in HBM, and the gate reads it from there.
//
// The gate (K3): E = H_o P_sub and S = E H_o^T + sigma^2 I on the fp64 matrix cores (v_mfma_f64_16x16x4_f64; operand layout as in
// k_gain.h: A lane -> (row lane & 15, k lane >> 4), B lane -> (k lane >> 4, column lane & 15), D register r of a lane -> (row
// (lane >> 4) + 4 r, column lane & 15)).  A wavefront owns a strip of 16 projected rows; it walks the 6M columns in chunks of 16:
// the chunk's tile of E (16 x 16, product depth 6M, P_sub gathered from P through the track's slots) goes through a tile of LDS
// of its own and is multiplied at once into the strip's tiles of the LOWER triangle of S, which stay in accumulators until the
// strip is done.  E never exists as a whole.  S (packed lower triangle, the residual r_o appended as one more row) is then
// eliminated in LDS by all threads, one barrier per pivot: gamma = sum_k S[q][k]^2 / S[k][k] over the eliminated extra row, a
// pivot that is not > 0 is the not-SPD verdict (code 2), as k_feature reports it.
//
// No wait on another workgroup, no atomics, every loop bounded by M.  fp64 only (the host refuses wide tracks on an f32 context).
#pragma once
#include <hip/hip_runtime.h>
#include "wave_ops.h"
#include "k_feature.h"            // FeatureArgs, feature_verdict, view_row.h

namespace msckf {

constexpr int FEATW_T = 256;      // threads of a workgroup: one per measurement row (2M <= 128) in K1, four wavefronts in the gate
constexpr int FEATW_MAXM = 64;    // = MSCKF_MAX_TRACK_WIDE (msckf_abi.hip asserts it)
constexpr int FEATW_ET_LD = 17;   // row stride of a wavefront's E tile (odd: the A operand's column walk is conflict free)

struct FeatureWideArgs {
    FeatureArgs a;                // as k_feature takes them (split, f0 unused)
    const int* list;              // [gridDim.x] sorted indices of the batch's wide tracks: workgroup b takes track list[b]
};

// LDS carve-up (doubles), sized for FEATW_MAXM views whatever the track holds: 2 V^2 + 43.5 V + 1105 at V views
//   (= 12081 doubles = 94.4 KiB at 64 -- one workgroup per CU; the 160 KiB of a CU would hold V = 88)
struct FeatWideLayout {
    static constexpr int V = FEATW_MAXM;
    static constexpr int slot = 0;                        // int [V]
    static constexpr int A = slot + V / 2;                // [2V][6]  OC-projected clone block rows (D)
    static constexpr int Vr = A + 2 * V * 6;              // [2V][3]  H_f rows (K1), then the Householder vectors' rows
    static constexpr int res = Vr + 2 * V * 3;            // [2V]     r
    static constexpr int ro = res + 2 * V;                // [2V]     r_o = Q^T r
    static constexpr int Z = ro + 2 * V;                  // [3][6V]
    static constexpr int misc = Z + 3 * 6 * V;            // T (6 doubles), rank (int at [8])
    static constexpr int Et = misc + 16;                  // [4][16][17] a wavefront's tile of E
    static constexpr int S = Et + 4 * 16 * FEATW_ET_LD;   // packed lower triangle of [S ; r_o^T]: (2V + 1)(2V + 2) / 2
    static constexpr int total = S + (2 * V + 1) * (2 * V + 2) / 2;
};
constexpr size_t FEATW_LDS_BYTES = (size_t)FeatWideLayout::total * 8;
static_assert(FEATW_LDS_BYTES <= 160 * 1024 - 1024, "k_feature_wide: LDS of one workgroup");

__global__ __launch_bounds__(FEATW_T) void k_feature_wide(FeatureWideArgs w) {
    typedef double v4d_ __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const FeatureArgs& p = w.a;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int f = w.list[blockIdx.x];
    const int v0 = p.view_ptr[f];
    const int M = p.view_ptr[f + 1] - v0;
    if (blockIdx.x == 0 && t < 8) static_cast<double*>(p.stack)[p.zero_idx + t] = 0.0;   // the stack's zero words (as k_feature's track 0)
    if (M < 1 || M > FEATW_MAXM) {            // (never sent by the host: nothing below may index past the carve-up)
        if (t == 0) feature_verdict(p, f, 0, 0.0, 0);
        return;
    }
    const int R2 = 2 * M, C6 = 6 * M;
    int* sSlot = reinterpret_cast<int*>(smem + FeatWideLayout::slot);
    double* sA = smem + FeatWideLayout::A;
    double* sV = smem + FeatWideLayout::Vr;
    double* sRes = smem + FeatWideLayout::res;
    double* sRo = smem + FeatWideLayout::ro;
    double* sZ = smem + FeatWideLayout::Z;
    double* sMisc = smem + FeatWideLayout::misc;
    double* sEt = smem + FeatWideLayout::Et + wv * 16 * FEATW_ET_LD;
    double* sS = smem + FeatWideLayout::S;

    if (p.select && !(p.select[f] & 1)) {      // not in valid_features (MSCKF.py:453-455): no rows, not a rejection
        if (t == 0) feature_verdict(p, f, 0, 0.0, 3);
        return;
    }
    long long tq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.stamps) tq[0] = wall_clock64();
    // ---------------- K1: one measurement row per thread (view_row.h) ------------
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
    }
    __syncthreads();
    if (p.stamps) tq[1] = wall_clock64();
    // ---------------- K2: column-pivoted Householder QR of H_f, the first wavefront with rows `lane` and `lane + 64` per lane -----
    // After step k row k holds R_kk; rows >= rank span the left null space.  The rank decision is k_feature's.
    if (wv == 0) {
        const int rw[2] = {lane, lane + 64};
        const bool in[2] = {rw[0] < R2, rw[1] < R2};
        double c0[2], c1[2], c2[2], rs[2];
        double vv0[2] = {0.0, 0.0}, vv1[2] = {0.0, 0.0}, vv2[2] = {0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            c0[s] = in[s] ? sV[rw[s] * 3 + 0] : 0.0; c1[s] = in[s] ? sV[rw[s] * 3 + 1] : 0.0; c2[s] = in[s] ? sV[rw[s] * 3 + 2] : 0.0;
            rs[s] = in[s] ? sRes[rw[s]] : 0.0;
        }
        auto wsum = [&](const double (&x)[2]) -> double { return wave_sum(x[0] + x[1]); };
        double beta0 = 0, beta1 = 0, beta2 = 0;
        int rank = 0;
        double r00 = 0.0;
        const double tol_scale = 2.220446049250313e-16 * (double)(R2 > 3 ? R2 : 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool act[2] = {in[0] && rw[0] >= k, in[1]};
            double x[2];
            x[0] = act[0] ? c0[0] * c0[0] : 0.0; x[1] = act[1] ? c0[1] * c0[1] : 0.0;
            double n0 = wsum(x), n1 = -1.0, n2 = -1.0;
            if (k < 2) { x[0] = act[0] ? c1[0] * c1[0] : 0.0; x[1] = act[1] ? c1[1] * c1[1] : 0.0; n1 = wsum(x); }
            if (k < 1) { x[0] = act[0] ? c2[0] * c2[0] : 0.0; x[1] = act[1] ? c2[1] * c2[1] : 0.0; n2 = wsum(x); }
            // pivot: bring the largest remaining column to the front (c0)
            if (n1 > n0 && n1 >= n2) {
#pragma unroll
                for (int s = 0; s < 2; ++s) { const double t_ = c0[s]; c0[s] = c1[s]; c1[s] = t_; }
                n0 = n1;
            } else if (n2 > n0 && n2 > n1) {
#pragma unroll
                for (int s = 0; s < 2; ++s) { const double t_ = c0[s]; c0[s] = c2[s]; c2[s] = t_; }
                n0 = n2;
            }
            const double ry = fast_rsqrt(n0);
            const double nrm = n0 * ry;
            if (k == 0) r00 = nrm;
            if (!(nrm > tol_scale * r00) || nrm == 0.0) break;   // numerically rank deficient (a zero column gives NaN and leaves here)
            const double xk = lane_bcast(c0[0], k);
            const double alpha = (xk > 0.0) ? -nrm : nrm;
            double vk[2];
            vk[0] = act[0] ? ((lane == k) ? (xk - alpha) : c0[0]) : 0.0;
            vk[1] = act[1] ? c0[1] : 0.0;
            const double beta = ry * fast_rcp(nrm + fabs(xk));   // 1 / (nrm (nrm + |xk|))
            if (k < 2) {
                x[0] = vk[0] * (act[0] ? c1[0] : 0.0); x[1] = vk[1] * (act[1] ? c1[1] : 0.0);
                const double d1 = wsum(x);
#pragma unroll
                for (int s = 0; s < 2; ++s) if (act[s]) c1[s] -= beta * d1 * vk[s];
            }
            if (k < 1) {
                x[0] = vk[0] * (act[0] ? c2[0] : 0.0); x[1] = vk[1] * (act[1] ? c2[1] : 0.0);
                const double d2 = wsum(x);
#pragma unroll
                for (int s = 0; s < 2; ++s) if (act[s]) c2[s] -= beta * d2 * vk[s];
            }
            if (k == 0) { vv0[0] = vk[0]; vv0[1] = vk[1]; beta0 = beta; }
            else if (k == 1) { vv1[0] = vk[0]; vv1[1] = vk[1]; beta1 = beta; }
            else { vv2[0] = vk[0]; vv2[1] = vk[1]; beta2 = beta; }
            rank = k + 1;
#pragma unroll
            for (int s = 0; s < 2; ++s) { c0[s] = c1[s]; c1[s] = c2[s]; c2[s] = 0.0; }
        }
        // T of the compact WY form Q = I - V T V^T (forward, columnwise)
        double x[2];
        x[0] = vv0[0] * vv1[0]; x[1] = vv0[1] * vv1[1]; const double v01 = wsum(x);
        x[0] = vv0[0] * vv2[0]; x[1] = vv0[1] * vv2[1]; const double v02 = wsum(x);
        x[0] = vv1[0] * vv2[0]; x[1] = vv1[1] * vv2[1]; const double v12 = wsum(x);
        const double T00 = beta0, T11 = beta1, T22 = beta2;
        const double T01 = -beta1 * T00 * v01;
        const double T02 = -beta2 * (T00 * v02 + T01 * v12);
        const double T12 = -beta2 * T11 * v12;
        // residual: r_o = r - V T^T V^T r
        x[0] = vv0[0] * rs[0]; x[1] = vv0[1] * rs[1]; const double wr0 = wsum(x);
        x[0] = vv1[0] * rs[0]; x[1] = vv1[1] * rs[1]; const double wr1 = wsum(x);
        x[0] = vv2[0] * rs[0]; x[1] = vv2[1] * rs[1]; const double wr2 = wsum(x);
        const double zr0 = T00 * wr0;
        const double zr1 = T01 * wr0 + T11 * wr1;
        const double zr2 = T02 * wr0 + T12 * wr1 + T22 * wr2;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (in[s]) {
                sV[rw[s] * 3 + 0] = vv0[s]; sV[rw[s] * 3 + 1] = vv1[s]; sV[rw[s] * 3 + 2] = vv2[s];
                sRo[rw[s]] = rs[s] - (vv0[s] * zr0 + vv1[s] * zr1 + vv2[s] * zr2);
            }
        }
        if (lane == 0) {
            sMisc[0] = T00; sMisc[1] = T01; sMisc[2] = T02; sMisc[3] = T11; sMisc[4] = T12; sMisc[5] = T22;
            reinterpret_cast<int*>(sMisc + 8)[0] = rank;
        }
    }
    __syncthreads();
    const int rank = reinterpret_cast<const int*>(sMisc + 8)[0];
    const int q = R2 - rank;
    // W = V^T D (a view's two rows), Z = T^T W: one column of the 6M per thread and trip
    {
        const double T00 = sMisc[0], T01 = sMisc[1], T02 = sMisc[2], T11 = sMisc[3], T12 = sMisc[4], T22 = sMisc[5];
        for (int c = t; c < C6; c += FEATW_T) {
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
    if (p.stamps) tq[2] = wall_clock64();
    // ---------------- K4: rows rank .. 2M - 1 of [H_o | r_o] = [D - V Z | r_o], contiguous in the stack block -------------------
    const int ldb = C6 + 1;
    double* blk = static_cast<double*>(p.stack) + p.blk_off[f];
    {
        const int nel = q * ldb;
        for (int e = t; e < nel; e += FEATW_T) {
            const int L = e / ldb, cc = e - L * ldb;
            const int row = rank + L;
            double x;
            if (cc == C6) x = sRo[row];
            else {
                x = 0.0;
                x -= sV[row * 3 + 0] * sZ[cc];
                x -= sV[row * 3 + 1] * sZ[C6 + cc];
                x -= sV[row * 3 + 2] * sZ[2 * C6 + cc];
                const int vw = cc / 6;
                if (vw == (row >> 1)) x += sA[row * 6 + (cc - 6 * vw)];      // D: only the rows of the column's own view
            }
            blk[e] = x;
        }
        // [S ; r_o^T]: the extra row of the elimination
        for (int j = t; j < q; j += FEATW_T) sS[q * (q + 1) / 2 + j] = sRo[rank + j];
    }
    __threadfence_block();
    __syncthreads();                         // the gate reads the block this workgroup wrote
    if (p.stamps) tq[3] = wall_clock64();
    // ---------------- K3: S = H_o P_sub H_o^T + sigma^2 I, lower triangle, a strip of 16 rows per wavefront ---------------------
    {
        const int NI = (q + 15) >> 4, NC = (C6 + 15) >> 4;
        const int l15 = lane & 15, g4 = lane >> 4;
        constexpr int TRIP = 16;             // product steps of 4 whose loads are issued together
        for (int I = wv; I < NI; I += FEATW_T / 64) {
            v4d_ accS[8];
#pragma unroll
            for (int J = 0; J < 8; ++J) accS[J] = v4d_{0.0, 0.0, 0.0, 0.0};
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
                for (int J = 0; J < 8; ++J) {
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
            for (int J = 0; J < 8; ++J) {
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
    if (p.stamps) tq[4] = wall_clock64();
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
    if (p.stamps) tq[5] = wall_clock64();
    if (wv == 0) {
        double gam = 0.0;
        if (!bad) {
            double part = 0.0;
            for (int k = lane; k < q; k += 64) { const double y = sS[q * (q + 1) / 2 + k]; part += y * y / sS[k * (k + 1) / 2 + k]; }
            gam = wave_sum(part);
        }
        if (p.stamps) tq[6] = wall_clock64();
        bool ok = (q >= 1) && (bad == 0) && (q < p.n_chi2);
        if (ok) ok = (gam <= p.chi2[q]);
        if (lane == 0) {
            feature_verdict(p, f, rank, gam, ok ? 1 : (bad ? 2 : 0));     // 1 accepted, 0 rejected by the gate, 2 the gate matrix was not SPD
            if (p.stamps) { tq[7] = wall_clock64(); for (int i = 0; i < 8; ++i) p.stamps[8 * f + i] = tq[i]; }
        }
    }
}

}  // namespace msckf
