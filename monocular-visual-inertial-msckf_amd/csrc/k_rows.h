// Direct measurement rows on the resident filter: m <= 32 caller-given rows H over the leading n_cols of all d = 15 + 6N
// state columns (the IMU block included -- every kernel behind K5 is built for T_H = [0 | T]), a residual r and a full
// m x m noise matrix R.  The arithmetic is K6-K7's (k_gain.h, k_joseph_f64) carried over to a general R:
//     Y = P H^T (d x m)      S = H Y + R      S = L L^T
//     gamma = r^T S^-1 r     K = Y S^-1       dx = K r
//     W = K S - Y            Pn = P - K Y^T + W K^T      P_out = (Pn + Pn^T) / 2
// reference MSCKF.py:604-607 and :612-614 with R in the place of R_n: (I - K H) P (I - K H)^T + K R K^T expands to the Pn
// above, for any K, once S = H P H^T + R.  Always fp64.
//
// Two plain launches, and no workgroup waits for another inside one:
//   k_rows_y       one workgroup per 16-row slab of Y: the slab on the matrix cores (depth n_cols, so an IMU-only
//                  measurement costs 15 m d), then the slab's share H[:, slab] Y[slab, :] of S.
//   k_rows_update  one workgroup per PAIR of 16 x 16 tiles (I, J), I <= J, of P_out, as k_joseph_f64.  Every workgroup sums
//                  the partial S in slab order, factors the <= 32 x 32 S itself, forms gamma and so reads the same verdict
//                  from the same bits (a serial chain of ~3 m short steps per workgroup, 3 us at m = 3, ~30 us at m = 32,
//                  repeated by all of them in parallel: the price of a launch in which nobody waits for anybody); a
//                  rejected or not-SPD update ends there.  Else K and W for the 32 rows of its two
//                  tiles, both tiles of Pn over the depth 2 m, the halves of the symmetrisation meet in LDS and both
//                  mirror tiles leave bit-equal.  Diagonal workgroups write their 16 entries of dx.
// Nothing is accumulated with atomics: every sum has one owner and a fixed order, two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "k_gain.h"
#include "wave_ops.h"

namespace msckf {

constexpr int ROWS_MAX = 32;             // MSCKF_MAX_ROWS
constexpr int ROWS_LD = 33;              // LDS row stride of the 32-wide operands

struct RowsArgs {
    const double* P; int ldp;            // prior covariance (d x d)
    int d, m, n_cols, nsl;               // nsl: slabs that meet the first n_cols columns (partial S)
    const double* H;                     // [m][n_cols]
    const double* rz;                    // [m] the residual -- or the measured value z, with ...
    const double* nom; int nom_off;      // ... the resident nominal record: r = z - nom[nom_off + i]  (nom_off < 0: rz is r)
    const double* R;                     // [m][m]
    double crit;                         // applied iff gamma <= crit (+inf: not gated)
    double* Y;                           // [16 nt][32]: rows >= d and columns >= m are written as 0
    double* Spart;                       // [nsl][32][32]
    double* dx; double* Pout; int ldo;
    int* status;                         // [0]: 0 ok, 1 a pivot of S was not a positive normal number; [2]: the verdict as accepted count
    double* gate;                        // [0]: gamma
    int* status_h; double* gate_h;       // their mirrors in pinned host memory
};

// Y slab b = P[16 b .., :n_cols] H^T: four wavefronts cut the depth into contiguous quarters (as k_gemm_f64), two
// accumulators when m > 16; the partial tiles meet in LDS in wavefront order.
__global__ __launch_bounds__(256) void k_rows_y(RowsArgs g) {
    __shared__ double sAcc[4][2][4][64];
    __shared__ double sY[16][ROWS_LD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 16, r = lane & 15;
    const int ksteps = (g.n_cols + 3) / 4, kq = (ksteps + 3) / 4;       // MFMA steps per wavefront
    const int k_lo = wv * 4 * kq + (lane >> 4);
    const bool aok = m0 + r < g.d, b0ok = r < g.m, b1ok = 16 + r < g.m, two = g.m > 16;
    // clamped addresses and selected values: a guarded load compiles to an exec-mask branch each
    const size_t oa = aok ? (size_t)(m0 + r) * g.ldp : 0;
    const size_t ob0 = b0ok ? (size_t)r * g.n_cols : 0, ob1 = b1ok ? (size_t)(16 + r) * g.n_cols : 0;
    v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    constexpr int TRIP = 8;
    for (int s0 = 0; s0 < kq; s0 += TRIP) {
        double av[TRIP], bv0[TRIP], bv1[TRIP];
#pragma unroll
        for (int u = 0; u < TRIP; ++u) {
            const int k = k_lo + 4 * (s0 + u);
            const bool kok = (s0 + u < kq) && (k < g.n_cols);
            const int kk = kok ? k : 0;
            const double xa = g.P[oa + kk], x0 = g.H[ob0 + kk], x1 = g.H[ob1 + kk];
            av[u] = (aok && kok) ? xa : 0.0;
            bv0[u] = (b0ok && kok) ? x0 : 0.0;
            bv1[u] = (b1ok && kok) ? x1 : 0.0;
        }
#pragma unroll
        for (int u = 0; u < TRIP; ++u) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv0[u], acc0, 0, 0, 0);
        if (two) {
#pragma unroll
            for (int u = 0; u < TRIP; ++u) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv1[u], acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { sAcc[wv][0][i][lane] = acc0[i]; sAcc[wv][1][i][lane] = acc1[i]; }
    __syncthreads();
    // C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg; wavefront w finishes register w of both tiles
    {
        const int row = (lane >> 4) + 4 * wv, col = lane & 15;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            double x = 0.0;
#pragma unroll
            for (int w = 0; w < 4; ++w) x += sAcc[w][tt][wv][lane];
            sY[row][col + 16 * tt] = x;
            g.Y[(size_t)(m0 + row) * ROWS_MAX + col + 16 * tt] = x;
        }
    }
    if (m0 >= g.n_cols) return;          // (H is zero on this slab's columns: nothing to add to S)
    __syncthreads();
    const int i = threadIdx.x >> 3;
    if (i < g.m) {
        const int kn = min(16, g.n_cols - m0);
        for (int j = threadIdx.x & 7; j < g.m; j += 8) {
            double s = 0.0;
#pragma unroll 4
            for (int kk = 0; kk < kn; ++kk) s = fma(g.H[(size_t)i * g.n_cols + m0 + kk], sY[kk][j], s);
            g.Spart[(size_t)blockIdx.x * (ROWS_MAX * ROWS_MAX) + i * ROWS_MAX + j] = s;
        }
    }
}

__global__ __launch_bounds__(256) void k_rows_update(RowsArgs g) {
    __shared__ double sS[ROWS_MAX][ROWS_LD], sL[ROWS_MAX][ROWS_LD];
    __shared__ double sYt[ROWS_MAX][ROWS_LD], sK[ROWS_MAX][ROWS_LD], sW[ROWS_MAX][ROWS_LD];   // rows 0..15: tile row I, 16..31: J
    __shared__ double sT[2][16][17];
    __shared__ double sr[ROWS_MAX], sInv[ROWS_MAX], sCol[2][ROWS_MAX];
    __shared__ int sCtl[2];              // [1] the verdict
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int m0 = ti * 16, n0 = tj * 16, m = g.m;
    const bool first_wg = ti == 0 && tj == 0;

    // S = R + the slabs' partial sums, in slab order
    for (int idx = t; idx < ROWS_MAX * ROWS_MAX; idx += 256) {
        const int i = idx >> 5, j = idx & 31;
        double s = (i == j) ? 1.0 : 0.0;
        if (i < m && j < m) {
            s = g.R[i * m + j];
            // eight slabs' loads in flight, then their sum in slab order (a tail slot reads the last slab and adds 0.0)
            for (int b0 = 0; b0 < g.nsl; b0 += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double x = g.Spart[(size_t)min(b0 + u, g.nsl - 1) * (ROWS_MAX * ROWS_MAX) + idx];
                    v[u] = (b0 + u < g.nsl) ? x : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
        }
        sS[i][j] = s; sL[i][j] = s;
        // Y's rows of the two tiles (rows >= d and columns >= m are zeros in HBM)
        const int gi = (i < 16) ? m0 + i : n0 + i - 16;
        sYt[i][j] = g.Y[(size_t)gi * ROWS_MAX + j];
    }
    if (t < ROWS_MAX) {
        double x = 0.0;
        if (t < m) { x = g.rz[t]; if (g.nom_off >= 0) x -= g.nom[g.nom_off + t]; }    // r = z - nominal
        sr[t] = x;
        sInv[t] = 1.0;
    }
    __syncthreads();

    // S = L L^T, right-looking, the trailing matrix in registers: thread (ty, tx) holds S[ty + 8 q][tx].  Per pivot the owners of
    // column k lay it down in LDS (two buffers in turn), ONE barrier, and every thread scales its row and column entries itself.
    // Every thread reads the same pivot: the exit is uniform.  L's columns and 1 / l_kk go to sL / sInv for the solves below.
    bool bad = false;
    {
        const int tx = t & 31, ty = t >> 5;
        double a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = sS[ty + 8 * q][tx];
        for (int k = 0; k < m; ++k) {
            double* col = sCol[k & 1];
            if (tx == k) {
#pragma unroll
                for (int q = 0; q < 4; ++q) col[ty + 8 * q] = a[q];
            }
            __syncthreads();
            const double piv = col[k];
            if (!(piv >= 2.2250738585072014e-308 && piv <= 1.7976931348623157e308)) { bad = true; break; }
            const double dinv = fast_rsqrt(piv);
            const double cj = col[tx] * dinv;                        // l_jk of this thread's column
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = ty + 8 * q;
                const double ci = col[i] * dinv;
                if (i > k && tx > k) a[q] = fma(-ci, cj, a[q]);
            }
            if (t >= k && t < m) sL[t][k] = col[t] * dinv;           // column k, the diagonal included -> sqrt(piv)
            if (t == k) sInv[k] = dinv;
        }
        __syncthreads();
    }
    if (bad) {
        // (the accepted count 1 lets the outcome table reach its not-SPD row; dx and P_out are not written)
        if (first_wg && t == 0) {
            const double qnan = __longlong_as_double(0x7ff8000000000000ll);
            g.status[0] = 1; g.status[2] = 1; g.gate[0] = qnan;
            g.status_h[0] = 1; g.status_h[2] = 1; g.gate_h[0] = qnan;
        }
        return;
    }

    // gamma = |L^-1 r|^2: lane i holds element i, the pivot element travels by v_readlane
    if (wv == 0) {
        double w = (lane < ROWS_MAX) ? sr[lane] : 0.0, gam = 0.0;
        const int le = lane & 31;
        double inv = sInv[0], lij = sL[le][0];
        for (int j = 0; j < m; ++j) {
            const int jn = min(j + 1, m - 1);
            const double inv_n = sInv[jn], lij_n = sL[le][jn];
            const double wj = readlane_d(w, j) * inv;
            gam = fma(wj, wj, gam);
            if (lane > j && lane < m) w = fma(-lij, wj, w);
            inv = inv_n; lij = lij_n;
        }
        if (lane == 0) {
            const int applied = (gam <= g.crit) ? 1 : 0;             // (a NaN gamma fails the comparison: rejected)
            sCtl[1] = applied;
            if (first_wg) {
                g.status[0] = 0; g.status[2] = applied; g.gate[0] = gam;
                g.status_h[0] = 0; g.status_h[2] = applied; g.gate_h[0] = gam;
            }
        }
    }
    __syncthreads();
    if (!sCtl[1]) return;

    // K row = S^-1 (Y row): forward sweep with L, backward sweep with L^T.  Half a wavefront per row, lane e holds element e
    // (elements m.. are 0 and stay 0), four rows in flight per half; the pivot element travels by v_readlane.
    {
        const int e = lane & 31, half = lane >> 5, row0 = wv * 8 + half;       // rows row0 + 2 q
        double x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = sYt[row0 + 2 * q][e];
        // (the operands of step j + 1 are requested before step j's arithmetic: they do not depend on x)
        double inv = sInv[0], lej = sL[e][0];
        for (int j = 0; j < m; ++j) {
            const int jn = min(j + 1, m - 1);
            const double inv_n = sInv[jn], lej_n = sL[e][jn];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double lo = readlane_d(x[q], j), hi = readlane_d(x[q], 32 + j);
                const double xj = (half ? hi : lo) * inv;
                x[q] = (e > j && e < m) ? fma(-lej, xj, x[q]) : (e == j ? xj : x[q]);
            }
            inv = inv_n; lej = lej_n;
        }
        double lje = sL[m - 1][e];
        inv = sInv[m - 1];
        for (int j = m - 1; j >= 0; --j) {
            const int jn = max(j - 1, 0);
            const double inv_n = sInv[jn], lje_n = sL[jn][e];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double lo = readlane_d(x[q], j), hi = readlane_d(x[q], 32 + j);
                const double xj = (half ? hi : lo) * inv;
                x[q] = (e < j) ? fma(-lje, xj, x[q]) : (e == j ? xj : x[q]);
            }
            inv = inv_n; lje = lje_n;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) sK[row0 + 2 * q][e] = x[q];
    }
    __syncthreads();
    const int mp = (m + 3) & ~3;         // the depth in MFMA steps of 4: columns m..mp of K, W and Y are zeros
    // W = K S - Y (the residual of K = Y S^-1: the Joseph correction)
    {
        const int rr = t >> 3;
        for (int j = t & 7; j < mp; j += 8) {
            double s = 0.0;
#pragma unroll 4
            for (int k = 0; k < m; ++k) s = fma(sK[rr][k], sS[k][j], s);
            sW[rr][j] = s - sYt[rr][j];
        }
    }
    if (ti == tj && t < 16 && m0 + t < g.d) {
        double s = 0.0;
#pragma unroll 4
        for (int k = 0; k < m; ++k) s = fma(sK[t][k], sr[k], s);
        g.dx[m0 + t] = s;
    }
    __syncthreads();
    // tiles (I, J) and (J, I) of [-K | W] [Y | K]^T, depth 2 mp: wavefront 0 and wavefront 1
    if (wv < 2) {
        const int r = lane & 15, ra = wv == 0 ? r : 16 + r, rb = wv == 0 ? 16 + r : r;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        // (mp / 2 steps of depth 4, an even count: two steps' operands are read before the first product)
        for (int u = 0; u < mp / 2; u += 2) {
            double a[2], b[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = 4 * (u + h) + (lane >> 4);
                const bool first = k < mp;
                const int kk = first ? k : k - mp;
                a[h] = first ? -sK[ra][kk] : sW[ra][kk];
                b[h] = first ? sYt[rb][kk] : sK[rb][kk];
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[1], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) sT[wv][(lane >> 4) + 4 * i][lane & 15] = acc[i];
    }
    __syncthreads();
    {
        const int i = t >> 4, j = t & 15;
        const int gi = m0 + i, gj = n0 + j;
        if (gi < g.d && gj < g.d) {
            const double pn1 = g.P[(size_t)gi * g.ldp + gj] + sT[0][i][j];     // Pn[gi][gj]
            const double pn2 = g.P[(size_t)gj * g.ldp + gi] + sT[1][j][i];     // Pn[gj][gi]
            const double o = 0.5 * (pn1 + pn2);
            g.Pout[(size_t)gi * g.ldo + gj] = o;
            g.Pout[(size_t)gj * g.ldo + gi] = o;
        }
    }
}

}  // namespace msckf
