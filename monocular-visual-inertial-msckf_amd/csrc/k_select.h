// f1 -- feature selection and triangulation, the step in front of K1.
// Follows reference MSCKF.get_valid_features (src/msckf/MSCKF.py:458-495):
//   lost / too-short / parallax tests, intersection_of_lines (src/utils/geometry.py:274-303),
//   re-projection into the anchor clone (src/msckf/Camera.py:13-52) and the refresh of the
//   inverse-depth point (geometry.py:61-71).
// Eight lanes share one feature: each lane folds the lines i = sub, sub+8, ... into the 3x3
// normal matrix X and the right-hand side y, an 8-lane DPP sum combines them, and every lane
// then runs the same 3x3 Jacobi eigen-solve for pinv(X) (numpy's rcond = 1e-15 cut-off).
// HBM traffic: 7 doubles + 1 int per view in, 8 doubles + 1 byte per feature out; the kernel
// is launch-latency bound at MSCKF sizes (about 1 MB at 2000 x 10 views).
#pragma once
#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace msckf {

enum : unsigned char { SEL_VALID = 1, SEL_LOST = 2, SEL_REFRESHED = 4, SEL_REFINED = 8 };

struct SelectArgs {
    int F;
    const int* view_ptr;          // [F+1] CSR (sorted feature order)
    const int* obs_slot;          // [sumM] clone slot per view
    const double* line_base;      // [sumM*3]
    const double* line_dir;       // [sumM*3]
    const double* line_conf;      // [sumM]
    const int* lost_for;          // [F]
    const int* tracked_for;       // [F]
    const double* cam_R;          // [N*9]
    const double* cam_t;          // [N*3]
    double K[9], Kinv[9];
    int width, height, min_lost, min_tracked, use_parallax;
    double min_parallax_deg;
    unsigned char* flags;         // [F]
    double* idp_m;                // [F*3] refreshed in place
    double* idp_rho;              // [F]
    double* world;                // [F*3] triangulated point (NaN when none was computed)
};

// One Jacobi rotation annihilating a[p][q] of a symmetric 3x3 matrix (r is the third index).
#define MSCKF_JACOBI_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)            \
    do {                                                                                    \
        if (apq != 0.0) {                                                                   \
            const double th_ = (aqq - app) / (2.0 * apq);                                   \
            const double t_ = (th_ >= 0.0 ? 1.0 : -1.0) / (fabs(th_) + sqrt(th_ * th_ + 1.0)); \
            const double c_ = 1.0 / sqrt(t_ * t_ + 1.0), s_ = t_ * c_;                      \
            app -= t_ * apq;                                                                \
            aqq += t_ * apq;                                                                \
            apq = 0.0;                                                                      \
            const double rp_ = arp, rq_ = arq;                                              \
            arp = c_ * rp_ - s_ * rq_;                                                      \
            arq = s_ * rp_ + c_ * rq_;                                                      \
            double x_, y_;                                                                  \
            x_ = v0p; y_ = v0q; v0p = c_ * x_ - s_ * y_; v0q = s_ * x_ + c_ * y_;           \
            x_ = v1p; y_ = v1q; v1p = c_ * x_ - s_ * y_; v1q = s_ * x_ + c_ * y_;           \
            x_ = v2p; y_ = v2q; v2p = c_ * x_ - s_ * y_; v2q = s_ * x_ + c_ * y_;           \
        }                                                                                   \
    } while (0)

// Re-projection of the world point (wx, wy, wz) into the anchor clone (R, t) and, when it lands in front of the camera
// and inside the image, the refresh of feature f's inverse-depth point; false otherwise (nothing written).  Shared by
// k_select (the linear point) and k_select_refine (the refined one): `p` is either kernel's argument record.
template <typename Args>
__device__ __forceinline__ bool select_refresh(const Args& p, int f, const double* R, const double* t, double wx, double wy, double wz) {
    // W2Ci through the explicit inverse (geometry.py:35-37)
    const double i00 = R[4] * R[8] - R[5] * R[7], i01 = R[2] * R[7] - R[1] * R[8], i02 = R[1] * R[5] - R[2] * R[4];
    const double i10 = R[5] * R[6] - R[3] * R[8], i11 = R[0] * R[8] - R[2] * R[6], i12 = R[2] * R[3] - R[0] * R[5];
    const double i20 = R[3] * R[7] - R[4] * R[6], i21 = R[1] * R[6] - R[0] * R[7], i22 = R[0] * R[4] - R[1] * R[3];
    const double det = R[0] * i00 + R[1] * i10 + R[2] * i20;
    const double qx = wx - t[0], qy = wy - t[1], qz = wz - t[2];
    const double cx = (i00 * qx + i01 * qy + i02 * qz) / det;
    const double cy = (i10 * qx + i11 * qy + i12 * qz) / det;
    const double cz = (i20 * qx + i21 * qy + i22 * qz) / det;
    if (!(cz > 0.0)) return false;                                          // Camera.py:18
    const double hx = p.K[0] * cx + p.K[1] * cy + p.K[2] * cz;
    const double hy = p.K[3] * cx + p.K[4] * cy + p.K[5] * cz;
    const double hz = p.K[6] * cx + p.K[7] * cy + p.K[8] * cz;
    const double u = hx / hz, v = hy / hz;                                  // Camera.py:20-21
    if (u < 0.0 || u >= (double)p.width || v < 0.0 || v >= (double)p.height) return false;   // :24-26
    const double ex = p.Kinv[0] * u + p.Kinv[1] * v + p.Kinv[2];            // MSCKF.py:486
    const double ey = p.Kinv[3] * u + p.Kinv[4] * v + p.Kinv[5];
    const double ez = p.Kinv[6] * u + p.Kinv[7] * v + p.Kinv[8];
    const double gx = R[0] * ex + R[1] * ey + R[2] * ez;                    // :487
    const double gy = R[3] * ex + R[4] * ey + R[5] * ez;
    const double gz = R[6] * ex + R[7] * ey + R[8] * ez;
    // m = (cos phi sin theta, -sin phi, cos phi cos theta) = W_v / |W_v|  (geometry.py:64-67)
    const double gn = sqrt(gx * gx + gy * gy + gz * gz);
    p.idp_m[(size_t)f * 3 + 0] = gx / gn;
    p.idp_m[(size_t)f * 3 + 1] = gy / gn;
    p.idp_m[(size_t)f * 3 + 2] = gz / gn;
    p.idp_rho[f] = 1.0 / cz;                                                // geometry.py:61-62
    return true;
}

__global__ __launch_bounds__(256) void k_select(SelectArgs p) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int fr = gid >> 3, sub = threadIdx.x & 7;
    const bool live = fr < p.F;
    const int f = live ? fr : p.F - 1;            // idle groups shadow the last feature (DPP needs all lanes)
    const int v0 = p.view_ptr[f], v1 = p.view_ptr[f + 1];
    const int M = v1 - v0;

    const bool lost = p.lost_for[f] >= p.min_lost;                          // MSCKF.py:463-465
    const bool too_short = lost && p.tracked_for[f] < p.min_tracked;        // :467-469
    bool enough = false;
    if (p.use_parallax && M > 1) {                                          // :472-477
        const double* a = p.line_dir + (size_t)v0 * 3;
        const double* b = p.line_dir + (size_t)(v1 - 1) * 3;
        const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
        double dot = (a[0] / na) * (b[0] / nb) + (a[1] / na) * (b[1] / nb) + (a[2] / na) * (b[2] / nb);
        dot = fmin(1.0, fmax(-1.0, dot));                                   // geometry.py:249-253
        enough = acos(dot) * (180.0 / 3.14159265358979323846) > p.min_parallax_deg;
    }
    const bool tri = !too_short && (lost || enough);                        // :479

    // X = sum c (I - d d^T), y = sum c (I - d d^T) base          (geometry.py:285-297)
    double xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0, y0 = 0, y1 = 0, y2 = 0;
    if (tri) {
        for (int i = v0 + sub; i < v1; i += 8) {
            const double* dp = p.line_dir + (size_t)i * 3;
            const double* bp = p.line_base + (size_t)i * 3;
            const double c = p.line_conf[i];
            const double n = sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
            const double dx = dp[0] / n, dy = dp[1] / n, dz = dp[2] / n;
            const double db = dx * bp[0] + dy * bp[1] + dz * bp[2];
            xx += c * (1.0 - dx * dx); yy += c * (1.0 - dy * dy); zz += c * (1.0 - dz * dz);
            xy -= c * dx * dy; xz -= c * dx * dz; yz -= c * dy * dz;
            y0 += c * (bp[0] - dx * db); y1 += c * (bp[1] - dy * db); y2 += c * (bp[2] - dz * db);
        }
    }
    xx = row8_sum(xx); xy = row8_sum(xy); xz = row8_sum(xz);
    yy = row8_sum(yy); yz = row8_sum(yz); zz = row8_sum(zz);
    y0 = row8_sum(y0); y1 = row8_sum(y1); y2 = row8_sum(y2);
    if (!live || sub != 0) return;

    unsigned char flag = 0;
    double wx = __builtin_nan(""), wy = wx, wz = wx;
    if (too_short) {
        flag = SEL_LOST;
    } else if (tri) {
        flag = SEL_VALID | (lost ? SEL_LOST : 0);                           // :492-493
        // pinv(X) y through the eigen-decomposition X = V diag(l) V^T (cyclic Jacobi)
        double a00 = xx, a11 = yy, a22 = zz, a01 = xy, a02 = xz, a12 = yz;
        double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
        for (int sweep = 0; sweep < 12; ++sweep) {
            const double off = a01 * a01 + a02 * a02 + a12 * a12;
            if (off <= 1e-60 * (a00 * a00 + a11 * a11 + a22 * a22)) break;
            MSCKF_JACOBI_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            MSCKF_JACOBI_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            MSCKF_JACOBI_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        const double lmax = fmax(fabs(a00), fmax(fabs(a11), fabs(a22)));
        const double cut = 1e-15 * lmax;                                    // numpy.linalg.pinv rcond
        const double c0 = (fabs(a00) > cut) ? (v00 * y0 + v10 * y1 + v20 * y2) / a00 : 0.0;
        const double c1 = (fabs(a11) > cut) ? (v01 * y0 + v11 * y1 + v21 * y2) / a11 : 0.0;
        const double c2 = (fabs(a22) > cut) ? (v02 * y0 + v12 * y1 + v22 * y2) / a22 : 0.0;
        wx = v00 * c0 + v01 * c1 + v02 * c2;
        wy = v10 * c0 + v11 * c1 + v12 * c2;
        wz = v20 * c0 + v21 * c1 + v22 * c2;
        // anchor clone = clone of the first view (:481)
        const int s = p.obs_slot[v0];
        if (select_refresh(p, f, p.cam_R + (size_t)s * 9, p.cam_t + (size_t)s * 3, wx, wy, wz)) flag |= SEL_REFRESHED;
    }
    p.flags[f] = flag;
    p.world[(size_t)f * 3 + 0] = wx;
    p.world[(size_t)f * 3 + 1] = wy;
    p.world[(size_t)f * 3 + 2] = wz;
}

#undef MSCKF_JACOBI_ROT

// ---- nonlinear refinement of the triangulated point (optional second launch) ----
// The linear point of k_select is the meeting point of lines stored with the poses of the past; the update linearises
// about the resident poses.  For every track k_select flagged VALID | REFRESHED this kernel minimises the weighted
// reprojection cost c(x) = sum_i w_i |z_i - zhat_i(x)|^2 over x = (alpha, beta, rho), the inverse-depth point in the
// anchor clone, under the CURRENT poses: h_i = R_s^T (R_a [alpha, beta, 1]^T + rho (t_a - t_s)), zhat_i = h_xy / h_z,
// z_i = K^-1 [u, v, 1] dehomogenised, w_i = line_conf[i] (the weights of the linear step; view_sigma plays no part).
// Levenberg-Marquardt from the linear point, lambda0 = 1e-3, (A + lambda diag A) d = g solved by cofactors; a trial is
// accepted iff every h_z > 0, everything is finite and the cost is strictly smaller.  Accept: lambda <- max(lambda / 10,
// 1e-12), stop when max|d| <= 1e-9 max(1, max|x|).  Reject: lambda <- 10 lambda, stop when lambda > 1e8.  At most
// `iters` trials.  The result W = t_a + R_a [alpha, beta, 1]^T / rho is kept iff a trial was accepted, rho > 0 and W
// passes select_refresh (the anchor in-image test of k_select), which then rewrites m / rho; SEL_REFINED marks it.
// Everything else about the track -- bits 1, 2, 4, and the linear result of a track that is not kept -- stays.
// Eight lanes per feature as in k_select: each trial is one pass over the views (lane sub takes sub, sub + 8, ...) that
// folds A (6), g (3), the cost and the count of views with h_z <= 0, then 11 DPP sums; all eight lanes take the same
// step.  The DPP moves need every lane of the wavefront, so the trial loop is wave-uniform: it runs until every group
// of the wavefront has stopped, and stopped or idle groups fold nothing (zeros) and keep their state.  No LDS, no
// atomics, no wait between workgroups; the loop is bounded by `iters`.
// The iteration decides by comparing costs that differ in their last bits once it has converged, so WHERE it stops
// depends on every rounding.  Both functions are therefore compiled without contraction into fused multiply-adds and sum
// in a fixed order (per lane view by view, then the DPP tree): a host restatement written in the same order of
// operations takes the same decisions (tests/triangulate_ref.py), and two runs give the same bits.
struct SelectRefineArgs {
    int F, iters;
    const int* view_ptr;          // [F+1]
    const int* obs_slot;          // [sumM]
    const double* obs_uv;         // [sumM*2] pixels, as K1 reads them
    const double* line_conf;      // [sumM]
    const double* cam_R;          // [N*9] resident poses
    const double* cam_t;          // [N*3]
    double K[9], Kinv[9];
    int width, height;
    unsigned char* flags;         // [F] SEL_REFINED is or-ed in
    double* idp_m;                // [F*3] refreshed again where the refined point is kept
    double* idp_rho;              // [F]
    double* world;                // [F*3]
    double* cost0;                // [F] cost at the linear point (0 when not attempted)
    double* cost1;                // [F] cost at the result (= cost0 when it is not kept)
    int* trials;                  // [F]
};

struct RefineSums { double a00, a01, a02, a11, a12, a22, g0, g1, g2, c, bad; };

// A = sum w J^T J, g = sum w J^T e, c = sum w |e|^2 and the number of views with h_z <= 0 at (al, be, rho), summed over
// the group's eight lanes.  Every lane of the wavefront must call it; `act` false folds nothing.
__device__ __forceinline__ RefineSums refine_eval(const SelectRefineArgs& p, bool act, int v0, int v1, int sub,
                                                  const double* Ra, const double* ta, double al, double be, double rho) {
#pragma clang fp contract(off)
    RefineSums s{};
    if (act) {
        const double rx = Ra[0] * al + Ra[1] * be + Ra[2];      // the anchor's ray R_a [al, be, 1]
        const double ry = Ra[3] * al + Ra[4] * be + Ra[5];
        const double rz = Ra[6] * al + Ra[7] * be + Ra[8];
        for (int i = v0 + sub; i < v1; i += 8) {
            const int sl = p.obs_slot[i];
            const double* R = p.cam_R + (size_t)sl * 9;
            const double* t = p.cam_t + (size_t)sl * 3;
            const double u = p.obs_uv[2 * (size_t)i], v = p.obs_uv[2 * (size_t)i + 1];
            const double w = p.line_conf[i];
            const double zx = p.Kinv[0] * u + p.Kinv[1] * v + p.Kinv[2];
            const double zy = p.Kinv[3] * u + p.Kinv[4] * v + p.Kinv[5];
            const double zw = p.Kinv[6] * u + p.Kinv[7] * v + p.Kinv[8];
            const double dx = ta[0] - t[0], dy = ta[1] - t[1], dz = ta[2] - t[2];
            const double yx = rx + rho * dx, yy = ry + rho * dy, yz = rz + rho * dz;
            const double hx = R[0] * yx + R[3] * yy + R[6] * yz;            // h = R_s^T y
            const double hy = R[1] * yx + R[4] * yy + R[7] * yz;
            const double hz = R[2] * yx + R[5] * yy + R[8] * yz;
            // dh/dalpha, dh/dbeta = R_s^T (columns 0, 1 of R_a), dh/drho = R_s^T (t_a - t_s)
            const double p0x = R[0] * Ra[0] + R[3] * Ra[3] + R[6] * Ra[6];
            const double p0y = R[1] * Ra[0] + R[4] * Ra[3] + R[7] * Ra[6];
            const double p0z = R[2] * Ra[0] + R[5] * Ra[3] + R[8] * Ra[6];
            const double p1x = R[0] * Ra[1] + R[3] * Ra[4] + R[6] * Ra[7];
            const double p1y = R[1] * Ra[1] + R[4] * Ra[4] + R[7] * Ra[7];
            const double p1z = R[2] * Ra[1] + R[5] * Ra[4] + R[8] * Ra[7];
            const double p2x = R[0] * dx + R[3] * dy + R[6] * dz;
            const double p2y = R[1] * dx + R[4] * dy + R[7] * dz;
            const double p2z = R[2] * dx + R[5] * dy + R[8] * dz;
            const double zh0 = hx / hz, zh1 = hy / hz;
            const double e0 = zx / zw - zh0, e1 = zy / zw - zh1;
            const double j00 = (p0x - zh0 * p0z) / hz, j01 = (p1x - zh0 * p1z) / hz, j02 = (p2x - zh0 * p2z) / hz;
            const double j10 = (p0y - zh1 * p0z) / hz, j11 = (p1y - zh1 * p1z) / hz, j12 = (p2y - zh1 * p2z) / hz;
            s.a00 += w * (j00 * j00 + j10 * j10); s.a01 += w * (j00 * j01 + j10 * j11); s.a02 += w * (j00 * j02 + j10 * j12);
            s.a11 += w * (j01 * j01 + j11 * j11); s.a12 += w * (j01 * j02 + j11 * j12); s.a22 += w * (j02 * j02 + j12 * j12);
            s.g0 += w * (j00 * e0 + j10 * e1); s.g1 += w * (j01 * e0 + j11 * e1); s.g2 += w * (j02 * e0 + j12 * e1);
            s.c += w * (e0 * e0 + e1 * e1);
            if (!(hz > 0.0)) s.bad += 1.0;
        }
    }
    s.a00 = row8_sum(s.a00); s.a01 = row8_sum(s.a01); s.a02 = row8_sum(s.a02);
    s.a11 = row8_sum(s.a11); s.a12 = row8_sum(s.a12); s.a22 = row8_sum(s.a22);
    s.g0 = row8_sum(s.g0); s.g1 = row8_sum(s.g1); s.g2 = row8_sum(s.g2);
    s.c = row8_sum(s.c); s.bad = row8_sum(s.bad);
    return s;
}

__global__ __launch_bounds__(256) void k_select_refine(SelectRefineArgs p) {
#pragma clang fp contract(off)
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int fr = gid >> 3, sub = threadIdx.x & 7;
    const bool live = fr < p.F;
    const int f = live ? fr : p.F - 1;            // idle groups shadow the last feature and fold nothing
    const int v0 = p.view_ptr[f], v1 = p.view_ptr[f + 1];
    const unsigned char flag = p.flags[f];
    const double* Ra = p.cam_R + (size_t)p.obs_slot[v0] * 9;
    const double* ta = p.cam_t + (size_t)p.obs_slot[v0] * 3;

    // start: the linear point in the anchor frame, C = R_a^T (W - t_a), x0 = (C_x / C_z, C_y / C_z, 1 / C_z)
    const double qx = p.world[(size_t)f * 3 + 0] - ta[0], qy = p.world[(size_t)f * 3 + 1] - ta[1], qz = p.world[(size_t)f * 3 + 2] - ta[2];
    const double cx = Ra[0] * qx + Ra[3] * qy + Ra[6] * qz;
    const double cy = Ra[1] * qx + Ra[4] * qy + Ra[7] * qz;
    const double cz = Ra[2] * qx + Ra[5] * qy + Ra[8] * qz;
    double al = cx / cz, be = cy / cz, rho = 1.0 / cz;
    const bool cand = live && (flag & (SEL_VALID | SEL_REFRESHED)) == (SEL_VALID | SEL_REFRESHED) && cz > 0.0;
    RefineSums cur = refine_eval(p, cand, v0, v1, sub, Ra, ta, al, be, rho);
    const bool attempted = cand && cur.bad == 0.0;          // feasible start
    const double c0 = cur.c;
    bool run = attempted, moved = false;
    double lam = 1e-3;
    int trials = 0;
    for (int it = 0; it < p.iters; ++it) {
        if (!__any(run)) break;                             // wave-uniform: every group of the wavefront has stopped
        const double m00 = cur.a00 + lam * cur.a00, m11 = cur.a11 + lam * cur.a11, m22 = cur.a22 + lam * cur.a22;
        const double m01 = cur.a01, m02 = cur.a02, m12 = cur.a12;
        const double k00 = m11 * m22 - m12 * m12, k01 = m02 * m12 - m01 * m22, k02 = m01 * m12 - m02 * m11;
        const double k11 = m00 * m22 - m02 * m02, k12 = m01 * m02 - m00 * m12, k22 = m00 * m11 - m01 * m01;
        const double det = m00 * k00 + m01 * k01 + m02 * k02;
        const double d0 = (k00 * cur.g0 + k01 * cur.g1 + k02 * cur.g2) / det;
        const double d1 = (k01 * cur.g0 + k11 * cur.g1 + k12 * cur.g2) / det;
        const double d2 = (k02 * cur.g0 + k12 * cur.g1 + k22 * cur.g2) / det;
        const double tal = al + d0, tbe = be + d1, trho = rho + d2;
        const RefineSums tr = refine_eval(p, run, v0, v1, sub, Ra, ta, tal, tbe, trho);
        if (run) {
            ++trials;
            const bool ok = tr.bad == 0.0 && isfinite(tal) && isfinite(tbe) && isfinite(trho) && isfinite(tr.c) && tr.c < cur.c;
            if (ok) {
                al = tal; be = tbe; rho = trho;
                cur = tr;
                moved = true;
                lam = fmax(lam / 10.0, 1e-12);
                const double dm = fmax(fabs(d0), fmax(fabs(d1), fabs(d2)));
                const double xm = fmax(fabs(al), fmax(fabs(be), fabs(rho)));
                if (dm <= 1e-9 * fmax(1.0, xm)) run = false;
            } else {
                lam *= 10.0;
                if (lam > 1e8) run = false;
            }
        }
    }
    if (!live || sub != 0) return;

    double c1 = c0;
    if (attempted && moved && rho > 0.0) {
        const double wx = ta[0] + (Ra[0] * al + Ra[1] * be + Ra[2]) / rho;
        const double wy = ta[1] + (Ra[3] * al + Ra[4] * be + Ra[5]) / rho;
        const double wz = ta[2] + (Ra[6] * al + Ra[7] * be + Ra[8]) / rho;
        if (select_refresh(p, f, Ra, ta, wx, wy, wz)) {
            p.world[(size_t)f * 3 + 0] = wx;
            p.world[(size_t)f * 3 + 1] = wy;
            p.world[(size_t)f * 3 + 2] = wz;
            p.flags[f] = flag | SEL_REFINED;
            c1 = cur.c;
        }
    }
    p.cost0[f] = attempted ? c0 : 0.0;
    p.cost1[f] = attempted ? c1 : 0.0;
    p.trials[f] = attempted ? trials : 0;
}

}  // namespace msckf
