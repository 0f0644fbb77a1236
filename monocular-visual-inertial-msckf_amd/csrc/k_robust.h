// Robust per-view weights in front of K1 (msckf_set_robust).  Not in the reference, whose only defence against
// a bad observation is the gate (MSCKF.py:562-579), all or nothing per track.
//
// One thread per view of the tracks [0, F) of the sorted arrays.  It forms the view's two residual components from K1's own
// point and observation (view_row.h's view_point: z / z_w - p_xy / p_z in normalised image coordinates, MSCKF.py:516,
// Camera.py:54-58) of the batch's current inverse-depth points and the resident poses, whitens their norm with the view's
// base weight b_v (sigma / sigma_v of msckf_set_view_sigma, else 1) and the global sigma,
//     s_v = b_v |e_v| / sigma,      w_v = b_v phi(s_v)      (robust_weight.h),
// and writes w_v where K1 reads FeatureArgs::obs_w from -- an array of the run's own: the base weights are read, never written,
// so a second run of the batch forms the same weights again.  A track the run skips (k_select's flags) gets w_v = b_v, s_v = 0.
//
// No LDS, no atomics, no wait on another workgroup.  The view's track is found by bisection of view_ptr (at most
// ceil(log2 F) steps; a track has at least one view, so the offsets are strictly ascending); that is the kernel's only loop.
#pragma once
#include <hip/hip_runtime.h>
#include "robust_weight.h"
#include "view_row.h"

namespace msckf {

struct RobustArgs {
    int F;                       // tracks (sorted order; the blocks of split tracks behind them are not K1's)
    int sumM;                    // their views: view_ptr[F]
    const int* view_ptr;         // [F+1] CSR, sorted order
    const double* obs_uv;        // [sumM*2]
    const int* obs_slot;         // [sumM]
    const double* obs_b;         // optional [sumM]: the base weights (null: every view at sigma)
    const double* idp_base;      // [F*3]
    const double* idp_m;         // [F*3]
    const double* idp_rho;       // [F]
    const double* cam_R;         // [N*9] R_W_Ci
    const double* cam_t;         // [N*3]
    const unsigned char* select; // optional [F] flags of k_select: tracks without bit 0 are skipped by K1
    double Kinv[9];
    double sigma;
    int loss;                    // kRobustHuber | kRobustCauchy
    double k, w_min;
    double* w;                   // [sumM] out: what K1 reads as obs_w
    double* s;                   // [sumM] out: the whitened residual norms
};

constexpr int ROBUST_THREADS = 256;

__global__ __launch_bounds__(ROBUST_THREADS) void k_robust(RobustArgs p) {
    const int o = blockIdx.x * ROBUST_THREADS + threadIdx.x;
    if (o >= p.sumM) return;
    // the track of view o: view_ptr[lo] <= o < view_ptr[hi] throughout (view_ptr[0] = 0, view_ptr[F] = sumM; neither end is read)
    int lo = 0, hi = p.F;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.view_ptr[mid] <= o) lo = mid; else hi = mid;
    }
    const int f = lo;
    const double b = p.obs_b ? p.obs_b[o] : 1.0;
    if (p.select && !(p.select[f] & 1)) { p.w[o] = b; p.s[o] = 0.0; return; }
    const int sl = p.obs_slot[o];
    const ViewPoint q = view_point(p.cam_R + 9 * sl, p.cam_t + 3 * sl, p.idp_base + 3 * f, p.idp_m + 3 * f, p.idp_rho[f], p.Kinv,
                                   p.obs_uv[2 * o], p.obs_uv[2 * o + 1]);
    const double ex = q.zx * q.izw - q.px * q.ia;           // view_row's two residuals
    const double ey = q.zy * q.izw - q.py * q.ia;
    const double sv = b * sqrt(ex * ex + ey * ey) / p.sigma;
    p.w[o] = b * robust_phi(p.loss, p.k, p.w_min, sv);
    p.s[o] = sv;
}

}  // namespace msckf
