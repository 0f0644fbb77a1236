// The robust loss in front of K1 (msckf_set_robust, k_robust.h): the weight function of one reweighting at the linearisation
// point and the check of its parameters.  Host and device code from one text, without a HIP header: k_robust.h calls it per view,
// msckf_abi.hip on the host (the parameter check, n_down), and tests/test_robust_weight_header.py compiles it with the host
// compiler (and its sanitizers) and walks the boundaries.  Not in the reference: its only defence is the gate (MSCKF.py:562-579).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define MSCKF_ROBUST_HD __host__ __device__
#else
#define MSCKF_ROBUST_HD
#endif

constexpr int kRobustOff = 0, kRobustHuber = 1, kRobustCauchy = 2;      // MSCKF_ROBUST_OFF / _HUBER / _CAUCHY

// msckf_robust_params as msckf_set_robust takes them: loss in 0..2, reserved 0, k finite and > 0, w_min in (0, 1]
inline bool robust_params_ok(int loss, int reserved, double k, double w_min) {
    if (loss < kRobustOff || loss > kRobustCauchy || reserved != 0) return false;
    if (!(std::isfinite(k) && k > 0.0)) return false;
    return w_min > 0.0 && w_min <= 1.0;               // (a NaN fails both)
}

// omega(s), the IRLS weight of a whitened residual norm s >= 0 on the SQUARED residual: Huber min(1, k / s) (exactly 1 up to
// s == k), Cauchy 1 / (1 + (s / k)^2)
MSCKF_ROBUST_HD inline double robust_omega(int loss, double k, double s) {
    if (loss == kRobustHuber) return s <= k ? 1.0 : k / s;
    if (loss == kRobustCauchy) { const double q = s / k; return 1.0 / (1.0 + q * q); }
    return 1.0;
}

// phi(s) = max(sqrt(omega(s)), w_min), the factor on the view's rows; 1 where s is not finite (K1 sees such a view as it does
// without the option) and with the loss off
MSCKF_ROBUST_HD inline double robust_phi(int loss, double k, double w_min, double s) {
    if (loss == kRobustOff || !std::isfinite(s)) return 1.0;
    const double r = std::sqrt(robust_omega(loss, k, s));
    return r > w_min ? r : w_min;
}
