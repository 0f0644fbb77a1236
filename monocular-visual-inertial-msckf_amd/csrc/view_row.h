// K1 of ONE view of one track: the point in the view's camera, the normalised observation, and one measurement row
// (view, image axis) of [r | H_x | H_f].   reference MSCKF.py:505-544, Camera.py:54-67
//
// Host and device code from one text, without a HIP header and on plain pointers and scalars: k_feature.h (a row per lane),
// k_feature_wide.h (a row per thread) and k_robust.h (the residual alone, through view_point) call it, and
// tests/test_view_row_header.py compiles it with the host compiler (and its sanitizers) against oracle.view_terms.
//
// The build contracts within one source expression only (-ffp-contract=on): every statement below stands as K1 has always
// written it, so the FMAs are the same wherever it is inlined.  A change to K1 is made HERE, once, and every expression that
// is regrouped moves the results of all three kernels alike.
#pragma once

#if defined(__HIPCC__)
#define MSCKF_VIEW_HD __host__ __device__ __forceinline__
#else
#define MSCKF_VIEW_HD inline
#endif

namespace msckf {

struct ViewPoint {
    double px, py, pz;           // Ci_f: the rho-scaled point in the view's camera
    double zx, zy;               // K^-1 [u v 1], first two components
    double ia, izw;              // 1 / p_z, 1 / z_w
};
struct ViewRow {
    double res;                  // r = z / z_w - p / p_z, this axis
    double a[6];                 // OC-projected clone block row (D)
    double h[3];                 // H_f row
};

// R, t: the view's clone R_W_Ci [9], position [3]; base, m [3], rho: the track's inverse-depth point; (u, v): the pixel
MSCKF_VIEW_HD ViewPoint view_point(const double* R, const double* t, const double* base, const double* m, double rho,
                                   const double* Kinv, double u, double v) {
    const double wx = rho * (base[0] - t[0]) + m[0];
    const double wy = rho * (base[1] - t[1]) + m[1];
    const double wz = rho * (base[2] - t[2]) + m[2];
    // Ci_f = R^T w   (MSCKF.py:516)
    const double px = R[0] * wx + R[3] * wy + R[6] * wz;
    const double py = R[1] * wx + R[4] * wy + R[7] * wz;
    const double pz = R[2] * wx + R[5] * wy + R[8] * wz;
    const double zx = Kinv[0] * u + Kinv[1] * v + Kinv[2];
    const double zy = Kinv[3] * u + Kinv[4] * v + Kinv[5];
    const double zw = Kinv[6] * u + Kinv[7] * v + Kinv[8];
    // (one division each for 1 / pz, 1 / zw and 1 / den; the other quotients of Camera.py are products with them: an IEEE
    //  division is ~15 instructions on the device, and ~1e-16 relative is what the products differ by)
    const double ia = 1.0 / pz;
    const double izw = 1.0 / zw;
    return ViewPoint{px, py, pz, zx, zy, ia, izw};
}

// Row `axis` (0: x, 1: y) of the view.  R0, t0: the clone's null-state pose; g [3]: gravity; w: the view's weight
// w_v = sigma / sigma_v, or null (every view at sigma).
MSCKF_VIEW_HD ViewRow view_row(const ViewPoint& q, const double* R, const double* t, const double* R0, const double* t0,
                               const double* g, int axis, const double* w) {
    double wv = 1.0;
    if (w) wv = *w;                             // (asked for here, used at the end)
    const double px = q.px, py = q.py, pz = q.pz, zx = q.zx, zy = q.zy, ia = q.ia, izw = q.izw;
    // W_f = R Ci_f + t (MSCKF.py:517)
    const double Wx = R[0] * px + R[1] * py + R[2] * pz + t[0];
    const double Wy = R[3] * px + R[4] * py + R[5] * pz + t[1];
    const double Wz = R[6] * px + R[7] * py + R[8] * pz + t[2];
    const double jb = -px * (ia * ia);
    const double jc = -py * (ia * ia);
    // u = [R0^T g ; (W_f - t0) x g]   (MSCKF.py:528-530)
    const double gx = g[0], gy = g[1], gz = g[2];
    const double u0 = R0[0] * gx + R0[3] * gy + R0[6] * gz;
    const double u1 = R0[1] * gx + R0[4] * gy + R0[7] * gz;
    const double u2 = R0[2] * gx + R0[5] * gy + R0[8] * gz;
    const double ex = Wx - t0[0], ey = Wy - t0[1], ez = Wz - t0[2];
    const double u3 = ey * gz - ez * gy;
    const double u4 = ez * gx - ex * gz;
    const double u5 = ex * gy - ey * gx;
    const double den = u0 * u0 + u1 * u1 + u2 * u2 + u3 * u3 + u4 * u4 + u5 * u5;
    double res, a0, a1, a2, a3, a4, a5, h0, h1, h2;
    double J0, J1, J2;   // this row of J (Camera.py:57-58)
    if (axis == 0) {
        res = zx * izw - px * ia;
        J0 = ia; J1 = 0.0; J2 = jb;
        a0 = -jb * py; a1 = -ia * pz + jb * px; a2 = ia * py;          // J skew(Ci_f), row 0
    } else {
        res = zy * izw - py * ia;
        J0 = 0.0; J1 = ia; J2 = jc;
        a0 = ia * pz - jc * py; a1 = jc * px; a2 = -ia * px;           // row 1
    }
    // H_f = J R^T (this row);  H_x[:,3:] = -H_f   (Camera.py:62,66; MSCKF.py:536)
    h0 = J0 * R[0] + J1 * R[1] + J2 * R[2];
    h1 = J0 * R[3] + J1 * R[4] + J2 * R[5];
    h2 = J0 * R[6] + J1 * R[7] + J2 * R[8];
    a3 = -h0; a4 = -h1; a5 = -h2;
    if (den > 1e-6) {      // observability-constrained projection (MSCKF.py:532-534)
        const double au = a0 * u0 + a1 * u1 + a2 * u2 + a3 * u3 + a4 * u4 + a5 * u5;
        const double aud = au * (1.0 / den);
        a0 -= aud * u0; a1 -= aud * u1; a2 -= aud * u2;
        a3 -= aud * u3; a4 -= aud * u4; a5 -= aud * u5;
    }
    // per-view noise: R_o = blockdiag(sigma_v^2 I_2) in whitened form -- the view's rows of r, H_x and H_f times
    // w_v = sigma / sigma_v, ONCE and in front of everything that forms Z, V or the gate's E: the null space behind K1 is that
    // of diag(w) H_f, so the projected noise is sigma^2 I again and nothing behind K1 knows of the weights
    if (w) {
        res *= wv;
        a0 *= wv; a1 *= wv; a2 *= wv; a3 *= wv; a4 *= wv; a5 *= wv;
        h0 *= wv; h1 *= wv; h2 *= wv;
    }
    return ViewRow{res, {a0, a1, a2, a3, a4, a5}, {h0, h1, h2}};
}

}  // namespace msckf
