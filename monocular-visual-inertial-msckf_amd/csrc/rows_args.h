// What msckf_run_rows / msckf_run_fix check on the host before anything is launched (k_rows.h).  Host code without a HIP header:
// tests/test_rows_args.py compiles it with the host compiler (and its sanitizers) and walks the boundaries.
#pragma once
#include <cstdint>
#include <cstring>

constexpr int kRowsMax = 32;             // MSCKF_MAX_ROWS

// R[m][m] equals its transpose bit for bit (a NaN equals a NaN of the same bits: a non-finite R is not an argument error, it
// ends at the pivot rule on the device)
inline bool rows_noise_symmetric(const double* R, int m) {
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < i; ++j) {
            std::uint64_t a, b;
            std::memcpy(&a, R + (std::size_t)i * m + j, 8);
            std::memcpy(&b, R + (std::size_t)j * m + i, 8);
            if (a != b) return false;
        }
    return true;
}

// 1 <= m <= 32 rows over the leading 1 <= n_cols <= d columns, no null pointer, R symmetric
inline bool rows_args_ok(int m, int n_cols, int d, const double* H, const double* r, const double* R) {
    if (m < 1 || m > kRowsMax || n_cols < 1 || n_cols > d) return false;
    if (!H || !r || !R) return false;
    return rows_noise_symmetric(R, m);
}
