// The nominal state beside the resident covariance: IMU integration, state injection and the augmentation's set-up on the
// device, so that a frame of the filter loop needs no host arithmetic and no round trip between two updates.
//   k_propagate_imu    MSCKF.process_imu for a BATCH of samples: IMU.integrate (src/msckf/IMU.py:78-100), Phi with the
//                      observability constraint and Q (src/msckf/MSCKF.py:166-237), P_II (:238), the product of the Phi's
//   k_propagate_strip  P_IC <- Phi_tot P_IC, P_CI <- P_IC^T (:241-242) and (P + P^T)/2 on the clone block (:244), once per batch
//   k_augment_imu      MSCKF.state_augmentation (:252-265): clone pose and J from the resident IMU state, then k_augment's arithmetic
//   k_inject           state half of MSCKF.correct (:616-661) from the dx K6-K7 left in HBM
//   k_compact_poses    pose half of MSCKF.remove_cameras on the device arrays
// What stays serial and why: a sample's Phi needs the state the previous sample left, and P_II the previous P_II, so the
// samples of a batch are a chain of ~10 dependent 15 x 15 steps each (one workgroup, everything in LDS, a barrier between
// steps).  Only the 15 x 6N strip is free of that chain: (Phi_n ... Phi_1) P_IC is formed once, spread over the strip's
// 16-column tiles.  All of it is latency-bound; the point is launches and round trips removed.
#pragma once
#include <hip/hip_runtime.h>
#include "k_state.h"

namespace msckf {

// The record in HBM: the doubles of msckf_nominal (include/msckf_mi355x.h) in its order, then one flag.
enum : int {
    NOM_R = 0, NOM_T = 9, NOM_V = 12, NOM_BG = 15, NOM_BA = 18, NOM_R0 = 21, NOM_T0 = 30, NOM_V0 = 33,
    NOM_G = 36, NOM_WP = 39, NOM_QC = 42, NOM_RIC = 186, NOM_TIC = 195, NOM_DOUBLES = 198,
    // != 0 once process_imu has run: the reference then holds the SAME objects as state and null state (MSCKF.py:247-248),
    // so an injection moves the null state with the state
    NOM_ALIAS = 198, NOM_RECORD = 199
};
constexpr int IMU_BATCH_MAX = 64;        // 7 doubles per sample in the kernel arguments (4 KB in all)

struct ImuBatchArgs {
    double* P; int d;                    // [d][d]; only the IMU block is touched here
    int n;
    double* nom;                         // the record, in place
    double* phi_tot;                     // [225] out: Phi_n ... Phi_1
    double s[IMU_BATCH_MAX * 7];         // RAW samples: gyro (3), acc (3), dt
};

__device__ __forceinline__ void nom_hat(const double* w, double* H) {      // geometry.py:222-235
    H[0] = 0.0; H[1] = -w[2]; H[2] = w[1];
    H[3] = w[2]; H[4] = 0.0; H[5] = -w[0];
    H[6] = -w[1]; H[7] = w[0]; H[8] = 0.0;
}
__device__ __forceinline__ void nom_mul33(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = fma(A[i * 3 + 2], B[6 + j], fma(A[i * 3 + 1], B[3 + j], A[i * 3] * B[j]));
}
__device__ __forceinline__ void nom_mulv(const double* A, const double* x, double* y) {
    for (int i = 0; i < 3; ++i) y[i] = fma(A[i * 3 + 2], x[2], fma(A[i * 3 + 1], x[1], A[i * 3] * x[0]));
}

// sm[]: what one sample's 15 x 15 steps read besides the matrices
enum : int { SM_HG = 0, SM_HW = 9, SM_RN = 18, SM_M1 = 27, SM_WW = 36, SM_RR = 45, SM_U = 54, SM_S = 57, SM_W1 = 60, SM_W2 = 63, SM_DT = 66, SM_N = 67 };

// One workgroup.  The 15 x 15 products are 225 threads x 15 fma in k_propagate's order; G (:200-212) is block-sparse
// (-I, I, -R, I), so Phi G, (..) G^T are sign flips and two 3-column products with R.
__global__ __launch_bounds__(256) void k_propagate_imu(ImuBatchArgs p) {
    __shared__ double st[NOM_RECORD], sm[SM_N];
    __shared__ double A[225], A2[225], Phi[225], X[225], Y[225], PII[225], TotA[225], TotB[225];
    const int tid = threadIdx.x, d = p.d;
    const int i = tid / 15, j = tid - i * 15;
    if (tid < NOM_RECORD) st[tid] = p.nom[tid];
    if (tid < 225) { PII[tid] = p.P[(size_t)i * d + j]; TotA[tid] = (i == j) ? 1.0 : 0.0; }
    double* Tot = TotA;
    double* Tot2 = TotB;
    __syncthreads();
    for (int k = 0; k < p.n; ++k) {
        if (tid == 0) {
            const double* q = p.s + 7 * k;
            const double dt = q[6];
            double gc[3], ac[3], w[3], aw[3], Rd[9], Rn[9], H[9], H2[9], tn[3], vn[3], x[3];
            for (int a = 0; a < 3; ++a) { gc[a] = q[a] - st[NOM_BG + a]; ac[a] = q[3 + a] - st[NOM_BA + a]; }    // MSCKF.py:166-167
            const double* R = st + NOM_R;
            // IMU.integrate, IMU.py:83-100
            for (int a = 0; a < 3; ++a)
                w[a] = gc[a] - fma(R[6 + a], st[NOM_WP + 2], fma(R[3 + a], st[NOM_WP + 1], R[a] * st[NOM_WP]));      // :83 (R^T w_planet)
            const double nw = sqrt(fma(w[2], w[2], fma(w[1], w[1], w[0] * w[0])));
            const double theta = nw * dt;
            for (int a = 0; a < 9; ++a) Rd[a] = (a % 4 == 0) ? 1.0 : 0.0;
            if (theta > 0.0) {                                                                                       // :85-88
                const double ax[3] = {w[0] / nw, w[1] / nw, w[2] / nw};
                nom_hat(ax, H);
                nom_mul33(H, H, H2);
                const double sn = sin(theta), cs = 1.0 - cos(theta);
                for (int a = 0; a < 9; ++a) Rd[a] = (Rd[a] + sn * H[a]) + cs * H2[a];
            }
            nom_mul33(R, Rd, Rn);                                                                                    // :92
            nom_mulv(R, ac, aw);
            for (int a = 0; a < 3; ++a) {
                aw[a] -= st[NOM_G + a];                                                                              // :94
                tn[a] = (st[NOM_T + a] + st[NOM_V + a] * dt) + (0.5 * aw[a]) * (dt * dt);                            // :96
                vn[a] = st[NOM_V + a] + aw[a] * dt;                                                                  // :97
            }
            // what F, G and the observability constraint read (MSCKF.py:182-233); null state = the record's at entry
            nom_hat(gc, sm + SM_HG);
            nom_hat(st + NOM_WP, sm + SM_HW);
            nom_hat(ac, H);
            nom_mul33(Rn, H, sm + SM_M1);                                         // R skew(acc), :186
            nom_mul33(sm + SM_HW, sm + SM_HW, sm + SM_WW);                        // (-W)(-W), :189
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b)                                       // R R_null^T, :221
                    sm[SM_RR + a * 3 + b] = fma(Rn[a * 3 + 2], st[NOM_R0 + b * 3 + 2], fma(Rn[a * 3 + 1], st[NOM_R0 + b * 3 + 1], Rn[a * 3] * st[NOM_R0 + b * 3]));
            nom_mulv(st + NOM_R0, st + NOM_G, sm + SM_U);                         // :223
            const double uu = fma(sm[SM_U + 2], sm[SM_U + 2], fma(sm[SM_U + 1], sm[SM_U + 1], sm[SM_U] * sm[SM_U]));
            for (int a = 0; a < 3; ++a) sm[SM_S + a] = sm[SM_U + a] / uu;         // :224
            for (int a = 0; a < 3; ++a) x[a] = st[NOM_V0 + a] - vn[a];
            nom_hat(x, H);
            nom_mulv(H, st + NOM_G, sm + SM_W1);                                  // :229
            for (int a = 0; a < 3; ++a) x[a] = (dt * st[NOM_V0 + a] + st[NOM_T0 + a]) - tn[a];
            nom_hat(x, H);
            nom_mulv(H, st + NOM_G, sm + SM_W2);                                  // :230
            sm[SM_DT] = dt;
            for (int a = 0; a < 9; ++a) { sm[SM_RN + a] = Rn[a]; st[NOM_R + a] = Rn[a]; st[NOM_R0 + a] = Rn[a]; }   // :99, :247
            for (int a = 0; a < 3; ++a) {
                st[NOM_T + a] = tn[a]; st[NOM_T0 + a] = tn[a];
                st[NOM_V + a] = vn[a]; st[NOM_V0 + a] = vn[a];                    // :100, :248
            }
            st[NOM_ALIAS] = 1.0;
        }
        __syncthreads();
        const double dt = sm[SM_DT];
        if (tid < 225) {                                                          // F dt, :179-192, :215
            const int bi = i / 3, bj = j / 3, r = i - 3 * bi, c = j - 3 * bj, e = r * 3 + c;
            double f = 0.0;
            if (bi == 0 && bj == 0) f = -sm[SM_HG + e];
            else if (bi == 0 && bj == 1) f = (r == c) ? -1.0 : 0.0;
            else if (bi == 2 && bj == 0) f = -sm[SM_M1 + e];
            else if (bi == 2 && bj == 2) f = -2.0 * sm[SM_HW + e];
            else if (bi == 2 && bj == 3) f = -sm[SM_RN + e];
            else if (bi == 2 && bj == 4) f = sm[SM_WW + e];
            else if (bi == 4 && bj == 2) f = (r == c) ? 1.0 : 0.0;
            A[tid] = f * dt;
        }
        __syncthreads();
        if (tid < 225) {
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < 15; ++l) s = fma(A[i * 15 + l], A[l * 15 + j], s);
            A2[tid] = s;                                                          // :216
        }
        __syncthreads();
        if (tid < 225) {
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < 15; ++l) s = fma(A2[i * 15 + l], A[l * 15 + j], s);                                  // :217
            Phi[tid] = ((((i == j) ? 1.0 : 0.0) + A[tid]) + 0.5 * A2[tid]) + (1.0 / 6.0) * s;                       // :218
        }
        __syncthreads();
        if (tid < 9) {
            Phi[(tid / 3) * 15 + tid % 3] = sm[SM_RR + tid];                      // :221
        } else if (tid < 15) {                                                    // :226-233, one thread per row
            const int a = tid - 9, row = (a < 3) ? 6 + a : 9 + a;
            const double wv = (a < 3) ? sm[SM_W1 + a] : sm[SM_W2 + a - 3];
            const double b0 = Phi[row * 15], b1 = Phi[row * 15 + 1], b2 = Phi[row * 15 + 2];
            const double m = fma(b2, sm[SM_U + 2], fma(b1, sm[SM_U + 1], b0 * sm[SM_U])) - wv;
            Phi[row * 15] = b0 - m * sm[SM_S];
            Phi[row * 15 + 1] = b1 - m * sm[SM_S + 1];
            Phi[row * 15 + 2] = b2 - m * sm[SM_S + 2];
        }
        __syncthreads();
        // Q = Phi G Qc G^T Phi^T dt, left to right as :237; X, Y are [15][12] here
        const int i12 = tid / 12, j12 = tid - i12 * 12;
        if (tid < 180) {                                                          // Phi G
            const int bj = j12 / 3, c = j12 - 3 * bj;
            double v = Phi[i12 * 15 + j12];
            if (bj == 0) v = -v;
            else if (bj == 2) v = -fma(Phi[i12 * 15 + 8], sm[SM_RN + 6 + c], fma(Phi[i12 * 15 + 7], sm[SM_RN + 3 + c], Phi[i12 * 15 + 6] * sm[SM_RN + c]));
            X[tid] = v;
        }
        __syncthreads();
        if (tid < 180) {                                                          // (Phi G) Qc
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < 12; ++l) s = fma(X[i12 * 12 + l], st[NOM_QC + l * 12 + j12], s);
            Y[tid] = s;
        }
        __syncthreads();
        if (tid < 180) {                                                          // (..) G^T
            const int bj = j12 / 3, c = j12 - 3 * bj;
            double v = Y[tid];
            if (bj == 0) v = -v;
            else if (bj == 2) v = -fma(Y[i12 * 12 + 8], sm[SM_RN + c * 3 + 2], fma(Y[i12 * 12 + 7], sm[SM_RN + c * 3 + 1], Y[i12 * 12 + 6] * sm[SM_RN + c * 3]));
            X[tid] = v;
        }
        __syncthreads();
        if (tid < 225) {
            double q = 0.0, t = 0.0, u = 0.0;
#pragma unroll
            for (int l = 0; l < 12; ++l) q = fma(X[i * 12 + l], Phi[j * 15 + l], q);                                 // (..) Phi^T
#pragma unroll
            for (int l = 0; l < 15; ++l) {
                t = fma(Phi[i * 15 + l], PII[l * 15 + j], t);                     // Phi P_II
                u = fma(Phi[i * 15 + l], Tot[l * 15 + j], u);                     // Phi Phi_tot
            }
            A2[tid] = q * dt;
            A[tid] = t;
            Tot2[tid] = u;
        }
        __syncthreads();
        if (tid < 225) {
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < 15; ++l) s = fma(A[i * 15 + l], Phi[j * 15 + l], s);
            Y[tid] = s + A2[tid];                                                 // :238
        }
        __syncthreads();
        if (tid < 225) PII[tid] = 0.5 * (Y[i * 15 + j] + Y[j * 15 + i]);          // :244 on the IMU block
        double* sw = Tot; Tot = Tot2; Tot2 = sw;
        __syncthreads();
    }
    if (tid < 225) { p.P[(size_t)i * d + j] = PII[tid]; p.phi_tot[tid] = Tot[tid]; }
    if (tid < NOM_RECORD) p.nom[tid] = st[tid];
}

// Grid (nb, 1 + nb), nb = 16-column tiles of the clone columns.  Row 0 of the grid: tile blockIdx.x of the strip,
// P_IC <- Phi_tot P_IC with the mirrored store (each workgroup owns its columns, reads them all before it writes).
// Rows 1 ..: the reference's whole-matrix (P + P^T)/2 on tile (blockIdx.y - 1, blockIdx.x) of the clone block, as
// k_symmetrize_tail.  k_augment and k_compact leave P_CC bit-symmetric (both mirror entries are the same expression /
// copies), which makes this pass the identity there; it is kept, once per batch instead of once per sample, because K7
// has several forms (k_gain_stream, k_gain_dense, the plain launches, f32) and not all of them promise bit-equal mirrors.
__global__ __launch_bounds__(256) void k_propagate_strip(double* P, int d, const double* phi_tot) {
    __shared__ double Tot[225];
    const int tid = threadIdx.x;
    if (blockIdx.y > 0) {
        const int jj = 15 + blockIdx.x * 16 + (tid & 15);
        const int ii = 15 + (blockIdx.y - 1) * 16 + (tid >> 4);
        if (ii < jj && jj < d) {
            const double v = 0.5 * (P[(size_t)ii * d + jj] + P[(size_t)jj * d + ii]);
            P[(size_t)ii * d + jj] = v;
            P[(size_t)jj * d + ii] = v;
        }
        return;
    }
    if (tid < 225) Tot[tid] = phi_tot[tid];
    __syncthreads();
    const int i = tid >> 4, j = 15 + blockIdx.x * 16 + (tid & 15);
    const bool mine = i < 15 && j < d;
    double s = 0.0;
    if (mine) {
#pragma unroll
        for (int k = 0; k < 15; ++k) s = fma(Tot[i * 15 + k], P[(size_t)k * d + j], s);
    }
    __syncthreads();
    if (mine) {
        P[(size_t)i * d + j] = s;                                                 // :241
        P[(size_t)j * d + i] = s;                                                 // :242
    }
}

struct AugmentImuArgs {
    const double* P; double* out; int d;
    const double* nom;
    double *camR, *camT, *camR0, *camT0; int slot;      // the new clone's slot (= N before the call)
};

// k_augment with J (MSCKF.py:258-261) and the clone's pose T_W_Ii T_I_C (:253) formed from the record.  Every workgroup
// forms J for itself (27 fma); workgroup 0 also writes the pose, which is the clone's null pose too (Camera.py:10-11).
__global__ __launch_bounds__(256) void k_augment_imu(AugmentImuArgs p) {
    __shared__ double J[90];
    const int tid = threadIdx.x;
    const double* R = p.nom + NOM_R;
    const double* Ric = p.nom + NOM_RIC;
    const double* tic = p.nom + NOM_TIC;
    if (tid < 90) {
        const int a = tid / 15, b = tid - a * 15;
        double v = 0.0;
        if (a < 3 && b < 3) v = Ric[b * 3 + a];                                   // :259
        else if (a >= 3 && b < 3 && a - 3 != b) {                                 // :260 skew(R t_I_C)
            const int r = a - 3, m = 3 - r - b;                                   // the component the entry holds
            const double w = fma(R[m * 3 + 2], tic[2], fma(R[m * 3 + 1], tic[1], R[m * 3] * tic[0]));
            v = ((b - r + 3) % 3 == 2) ? w : -w;                                  // (0,2) (1,0) (2,1) are +
        } else if (a >= 3 && b >= 12) v = (a - 3 == b - 12) ? 1.0 : 0.0;          // :261
        J[tid] = v;
    }
    if (blockIdx.x == 0 && tid >= 96 && tid < 108) {
        const int e = tid - 96;
        if (e < 9) {
            const int r = e / 3, c = e - 3 * r;
            const double v = fma(R[r * 3 + 2], Ric[6 + c], fma(R[r * 3 + 1], Ric[3 + c], R[r * 3] * Ric[c]));
            p.camR[(size_t)p.slot * 9 + e] = v;
            p.camR0[(size_t)p.slot * 9 + e] = v;
        } else {
            const int r = e - 9;
            const double v = fma(R[r * 3 + 2], tic[2], fma(R[r * 3 + 1], tic[1], R[r * 3] * tic[0])) + p.nom[NOM_T + r];
            p.camT[(size_t)p.slot * 3 + r] = v;
            p.camT0[(size_t)p.slot * 3 + r] = v;
        }
    }
    __syncthreads();
    const int d = p.d, n = d + 6;
    const int idx = blockIdx.x * 256 + tid;
    if (idx >= n * n) return;
    const int i = idx / n, j = idx - i * n;
    p.out[(size_t)i * n + j] = augment_entry(p.P, d, J, i, j);
}

// R <- polar(R Exp(dtheta)^T) (MSCKF.py:625-635, restated in inject.py).  The reference takes U V^T of an SVD, which is
// the orthogonal polar factor (unique: the matrices here are within rounding / 1e-7 of a rotation); Newton's iteration
// X <- (X + X^-T)/2 converges to it quadratically and is run until it stops moving.
__device__ inline void inject_rotation(double* R, const double* th) {
    const double n = sqrt(fma(th[2], th[2], fma(th[1], th[1], th[0] * th[0])));
    double E[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (!(n <= 1e-8)) {                                                           // numpy.isclose(n, 0): atol 1e-8
        double S[9], S2[9];
        nom_hat(th, S);
        nom_mul33(S, S, S2);
        const double a = sin(n) / n, b = (1.0 - cos(n)) / (n * n);
        for (int e = 0; e < 9; ++e) E[e] = (E[e] + a * S[e]) + b * S2[e];
    }
    double X[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) X[r * 3 + c] = fma(R[r * 3 + 2], E[c * 3 + 2], fma(R[r * 3 + 1], E[c * 3 + 1], R[r * 3] * E[c * 3]));   // R E^T
    for (int it = 0; it < 30; ++it) {
        double C[9];                                                              // cofactors: X^-T = C / det
        C[0] = X[4] * X[8] - X[5] * X[7]; C[1] = X[5] * X[6] - X[3] * X[8]; C[2] = X[3] * X[7] - X[4] * X[6];
        C[3] = X[2] * X[7] - X[1] * X[8]; C[4] = X[0] * X[8] - X[2] * X[6]; C[5] = X[1] * X[6] - X[0] * X[7];
        C[6] = X[1] * X[5] - X[2] * X[4]; C[7] = X[2] * X[3] - X[0] * X[5]; C[8] = X[0] * X[4] - X[1] * X[3];
        const double det = fma(X[2], C[2], fma(X[1], C[1], X[0] * C[0]));
        double delta = 0.0;
        for (int e = 0; e < 9; ++e) {
            const double v = 0.5 * (X[e] + C[e] / det);
            delta = fmax(delta, fabs(v - X[e]));
            X[e] = v;
        }
        if (delta < 1e-15) break;
    }
    for (int e = 0; e < 9; ++e) R[e] = X[e];
}

struct InjectArgs {
    const double* dx;                    // [15 + 6 N], as K6-K7 left it
    double* nom;
    double *camR, *camT, *camR0, *camT0; int N;
};

// One lane per pose: lane 0 the IMU (rotation, additive t, v, biases; :625-640), lane 1 + i clone i (:643-661), whose
// null pose is the pose itself (Camera.py:10-11).
__global__ __launch_bounds__(64) void k_inject(InjectArgs p) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx > p.N) return;
    double R[9];
    if (idx == 0) {
        double* s = p.nom;
        for (int e = 0; e < 9; ++e) R[e] = s[NOM_R + e];
        inject_rotation(R, p.dx);
        const bool alias = s[NOM_ALIAS] != 0.0;
        for (int e = 0; e < 9; ++e) { s[NOM_R + e] = R[e]; if (alias) s[NOM_R0 + e] = R[e]; }
        for (int e = 0; e < 3; ++e) {
            const double t = s[NOM_T + e] + p.dx[12 + e], v = s[NOM_V + e] + p.dx[6 + e];
            s[NOM_T + e] = t; s[NOM_V + e] = v;
            if (alias) { s[NOM_T0 + e] = t; s[NOM_V0 + e] = v; }
            s[NOM_BG + e] += p.dx[3 + e];
            s[NOM_BA + e] += p.dx[9 + e];
        }
        return;
    }
    const int c = idx - 1;
    const double* dc = p.dx + 15 + 6 * c;
    for (int e = 0; e < 9; ++e) R[e] = p.camR[(size_t)c * 9 + e];
    inject_rotation(R, dc);
    for (int e = 0; e < 9; ++e) { p.camR[(size_t)c * 9 + e] = R[e]; p.camR0[(size_t)c * 9 + e] = R[e]; }
    for (int e = 0; e < 3; ++e) {
        const double t = p.camT[(size_t)c * 3 + e] + dc[3 + e];
        p.camT[(size_t)c * 3 + e] = t; p.camT0[(size_t)c * 3 + e] = t;
    }
}

// Clone poses of the kept slots moved to the front, in place: everything is read into LDS before anything is written.
// keep[] is k_compact's index map (15 IMU entries, then 6 per kept clone).
__global__ __launch_bounds__(256) void k_compact_poses(double* camR, double* camT, double* camR0, double* camT0, const int* keep, int n_new) {
    extern __shared__ __attribute__((aligned(16))) double smem[];       // [n_new][24]
    for (int idx = threadIdx.x; idx < n_new * 24; idx += 256) {
        const int s = idx / 24, e = idx - s * 24, src = (keep[15 + 6 * s] - 15) / 6;
        smem[idx] = e < 9 ? camR[(size_t)src * 9 + e] : e < 12 ? camT[(size_t)src * 3 + e - 9]
                  : e < 21 ? camR0[(size_t)src * 9 + e - 12] : camT0[(size_t)src * 3 + e - 21];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_new * 24; idx += 256) {
        const int s = idx / 24, e = idx - s * 24;
        const double v = smem[idx];
        if (e < 9) camR[(size_t)s * 9 + e] = v;
        else if (e < 12) camT[(size_t)s * 3 + e - 9] = v;
        else if (e < 21) camR0[(size_t)s * 9 + e - 12] = v;
        else camT0[(size_t)s * 3 + e - 21] = v;
    }
}

struct ClonePoseArgs { double R[9], t[3]; double *camR, *camT, *camR0, *camT0; int slot; };

// msckf_augment on a context with a nominal state: the caller's pose goes into the device arrays (the host mirror is stale).
__global__ __launch_bounds__(64) void k_set_clone_pose(ClonePoseArgs p) {
    const int e = threadIdx.x;
    if (e < 9) { p.camR[(size_t)p.slot * 9 + e] = p.R[e]; p.camR0[(size_t)p.slot * 9 + e] = p.R[e]; }
    else if (e < 12) { p.camT[(size_t)p.slot * 3 + e - 9] = p.t[e - 9]; p.camT0[(size_t)p.slot * 3 + e - 9] = p.t[e - 9]; }
}

}  // namespace msckf
