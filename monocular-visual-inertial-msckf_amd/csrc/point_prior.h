// A Gaussian prior p ~ N(pbar, Sigma_p) on a track's point: three more rows in front of the null-space projection (K2),
//     [ H_f     ]     [ H_x ]     [ r                      ]       W^T W = Sigma_p^-1  (W = L^-1, Sigma_p = L L^T)
//     [ sigma W ]     [ 0   ]     [ sigma W (pbar - p_lin) ]       p_lin = idp_base + idp_m / idp_rho
// with noise sigma^2 I like every other row, so the left null space of the (2M + 3) x 3 block has 2M columns and the projected
// noise is sigma^2 I again.  It equals the EKF update with residual r - H_f (pbar - p_lin), Jacobian H_x and noise
// sigma^2 I + H_f Sigma_p H_f^T.  Not in the reference, whose tracks are all of unknown points (MSCKF.py:554-559).
//
// Units: the prior's columns are K1's H_f as it stands -- the block whose negative stands in the clone's position columns
// (Camera.py:62, :66, MSCKF.py:536) -- so a shift of the point and the opposite shift of every observing clone are the same
// thing to the filter; the reference's rho-scaled geometry is kept as it is.
//
// Host and device code from one text, without a HIP header and on plain pointers and scalars (as view_row.h, robust_weight.h):
// the check and the whitening run on the host when the priors are set, the rows are formed where K1 runs, from the base, m and
// rho K1 is about to use.  tests/test_point_prior_header.py compiles it with the host compiler (and its sanitizers) against
// tests/prior_ref.py.  Prior rows are not touched by per-view weights or by the robust loss: those belong to views.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MSCKF_PRIOR_HD __host__ __device__ inline
#else
#define MSCKF_PRIOR_HD inline
#endif

namespace msckf {

constexpr int kPriorAtMean = 1;          // MSCKF_PRIOR_AT_MEAN
constexpr int kMaxTrackPrior = 30;       // MSCKF_MAX_TRACK_PRIOR: 2M + 3 rows on 64 lanes

struct PriorRow {
    double res;                  // sigma W[k, :] . (pbar - p_lin)
    double h[3];                 // sigma W[k, :]            (the row's clone block is zero)
};

// The lower Cholesky factor L [9, row-major, upper part zero] of cov [9, row-major]; false where a pivot is not finite and > 0
inline bool point_prior_cholesky(const double* cov, double* L) {
    for (int i = 0; i < 9; ++i) L[i] = 0.0;
    for (int j = 0; j < 3; ++j) {
        double d = cov[3 * j + j];
        for (int k = 0; k < j; ++k) d -= L[3 * j + k] * L[3 * j + k];
        if (!(std::isfinite(d) && d > 0.0)) return false;
        const double ljj = std::sqrt(d);
        if (!(std::isfinite(ljj) && ljj > 0.0)) return false;
        L[3 * j + j] = ljj;
        for (int i = j + 1; i < 3; ++i) {
            double s = cov[3 * i + j];
            for (int k = 0; k < j; ++k) s -= L[3 * i + k] * L[3 * j + k];
            L[3 * i + j] = s / ljj;
        }
    }
    return true;
}

// mean [3], cov [9]: every entry finite, cov bitwise symmetric, its Cholesky factor with finite pivots > 0
inline bool point_prior_ok(const double* mean, const double* cov) {
    for (int i = 0; i < 3; ++i) if (!std::isfinite(mean[i])) return false;
    for (int i = 0; i < 9; ++i) if (!std::isfinite(cov[i])) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            std::uint64_t a, b;
            std::memcpy(&a, &cov[3 * i + j], 8);
            std::memcpy(&b, &cov[3 * j + i], 8);
            if (a != b) return false;
        }
    double L[9];
    return point_prior_cholesky(cov, L);
}

// W = L^-1 [9, row-major, lower triangular]: W^T W = cov^-1.  false where point_prior_cholesky fails or W is not finite
inline bool point_prior_whiten(const double* cov, double* W) {
    double L[9];
    if (!point_prior_cholesky(cov, L)) return false;
    for (int i = 0; i < 9; ++i) W[i] = 0.0;
    for (int j = 0; j < 3; ++j) {                   // forward substitution on the columns of I
        W[3 * j + j] = 1.0 / L[3 * j + j];
        for (int i = j + 1; i < 3; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s -= L[3 * i + k] * W[3 * k + j];
            W[3 * i + j] = s / L[3 * i + i];
        }
    }
    for (int i = 0; i < 9; ++i) if (!std::isfinite(W[i])) return false;
    return true;
}

// p_lin = base + m / rho, the point K1 linearises at
MSCKF_PRIOR_HD void point_prior_lin(const double* base, const double* m, double rho, double* p) {
    p[0] = base[0] + m[0] / rho;
    p[1] = base[1] + m[1] / rho;
    p[2] = base[2] + m[2] / rho;
}

// Row k (0..2) of the prior block: W [9] the whitening, mean = pbar [3], p_lin [3]
MSCKF_PRIOR_HD PriorRow point_prior_row(const double* W, const double* mean, const double* p_lin, double sigma, int k) {
    const double w0 = sigma * W[3 * k + 0], w1 = sigma * W[3 * k + 1], w2 = sigma * W[3 * k + 2];
    const double d0 = mean[0] - p_lin[0], d1 = mean[1] - p_lin[1], d2 = mean[2] - p_lin[2];
    const double res = w0 * d0 + w1 * d1 + w2 * d2;
    return PriorRow{res, {w0, w1, w2}};
}

// (pbar - p_lin)^T cov^-1 (pbar - p_lin) = |W (pbar - p_lin)|^2
MSCKF_PRIOR_HD double point_prior_distance(const double* W, const double* mean, const double* p_lin) {
    const double d0 = mean[0] - p_lin[0], d1 = mean[1] - p_lin[1], d2 = mean[2] - p_lin[2];
    const double y0 = W[0] * d0;
    const double y1 = W[3] * d0 + W[4] * d1;
    const double y2 = W[6] * d0 + W[7] * d1 + W[8] * d2;
    return y0 * y0 + y1 * y1 + y2 * y2;
}

// Linearise at the mean (MSCKF_PRIOR_AT_MEAN): rho' = 1 / |pbar - base|, m' = (pbar - base) rho', to be used in place of the
// track's m, rho by everything that forms the run's K1 terms; the stored m / rho are never overwritten.  false (m_out, rho_out
// untouched: the track keeps its own point) where |pbar - base| is not finite or is 0.
MSCKF_PRIOR_HD bool point_prior_at_mean(const double* mean, const double* base, double* m_out, double* rho_out) {
    const double d0 = mean[0] - base[0], d1 = mean[1] - base[1], d2 = mean[2] - base[2];
    const double n = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    if (!std::isfinite(n) || n == 0.0) return false;
    const double r = 1.0 / n;
    if (!std::isfinite(r)) return false;
    m_out[0] = d0 * r; m_out[1] = d1 * r; m_out[2] = d2 * r;
    *rho_out = r;
    return true;
}

}  // namespace msckf
