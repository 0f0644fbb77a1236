"""The host-side argument checks of msckf_run_rows / msckf_run_fix (csrc/rows_args.h) through a stand-alone driver built with the
host compiler from the header alone, under AddressSanitizer and UBSan: the boundaries of m and n_cols, null pointers, and the
bitwise symmetry of R (a NaN of equal bits on both sides is symmetric: a non-finite R is the device's business)."""
import os
import subprocess

import pytest

from conftest import ROOT

HEADER_DIR = os.path.join(ROOT, "monocular-visual-inertial-msckf_amd", "csrc")

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "rows_args.h"
int main() {
    const int d = 195;
    std::vector<double> H(32 * d, 1.0), r(32, 0.5), R(32 * 32, 0.0);
    for (int i = 0; i < 32; ++i) R[i * 32 + i] = 2.0;
    auto ok = [&](int m, int n, const double* h, const double* rr, const double* RR) { return (int)rows_args_ok(m, n, d, h, rr, RR); };
    std::printf("m0 %d\n", ok(0, 15, H.data(), r.data(), R.data()));
    std::printf("m1 %d\n", ok(1, 15, H.data(), r.data(), R.data()));
    std::printf("m32 %d\n", ok(32, d, H.data(), r.data(), R.data()));
    std::printf("m33 %d\n", ok(33, 15, H.data(), r.data(), R.data()));
    std::printf("n0 %d\n", ok(3, 0, H.data(), r.data(), R.data()));
    std::printf("n1 %d\n", ok(1, 1, H.data(), r.data(), R.data()));
    std::printf("nd %d\n", ok(1, d, H.data(), r.data(), R.data()));
    std::printf("nd1 %d\n", ok(1, d + 1, H.data(), r.data(), R.data()));
    std::printf("nullH %d\n", ok(3, 15, nullptr, r.data(), R.data()));
    std::printf("nullr %d\n", ok(3, 15, H.data(), nullptr, R.data()));
    std::printf("nullR %d\n", ok(3, 15, H.data(), r.data(), nullptr));
    // R of the last size that fits, exactly m * m doubles: the check reads no further
    for (int m : {1, 2, 17, 32}) {
        std::vector<double> S((size_t)m * m);
        for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) S[(size_t)i * m + j] = 1.0 / (1 + i + j) + (i == j);
        std::printf("sym%d %d\n", m, ok(m, 15, H.data(), r.data(), S.data()));
        if (m > 1) {
            S[(size_t)(m - 1) * m] = std::nextafter(S[m - 1], 2.0);          // one ulp off in the far corner
            std::printf("asym%d %d\n", m, ok(m, 15, H.data(), r.data(), S.data()));
            S[(size_t)(m - 1) * m] = S[m - 1] = std::nan("");                // the same NaN on both sides
            std::printf("nan%d %d\n", m, ok(m, 15, H.data(), r.data(), S.data()));
            S[m - 1] = 0.0; S[(size_t)(m - 1) * m] = -0.0;                   // 0.0 == -0.0, but not bit for bit
            std::printf("zero%d %d\n", m, ok(m, 15, H.data(), r.data(), S.data()));
        }
    }
    return 0;
}
"""

EXPECTED = {"m0": 0, "m1": 1, "m32": 1, "m33": 0, "n0": 0, "n1": 1, "nd": 1, "nd1": 0, "nullH": 0, "nullr": 0, "nullR": 0,
            "sym1": 1, **{f"{k}{m}": v for m in (2, 17, 32) for k, v in (("sym", 1), ("asym", 0), ("nan", 1), ("zero", 0))}}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("rows_args")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", HEADER_DIR, "-o", exe, src], check=True, timeout=120)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_argument_checks(rows):
    assert rows == EXPECTED


def test_header_and_abi_agree():
    hdr = open(os.path.join(ROOT, "include", "msckf_mi355x.h")).read()
    assert "#define MSCKF_MAX_ROWS 32" in hdr
    assert "constexpr int kRowsMax = 32;" in open(os.path.join(HEADER_DIR, "rows_args.h")).read()
    from msckf_amd import _ffi
    assert _ffi.MAX_ROWS == 32 and (_ffi.FIX_POSITION, _ffi.FIX_VELOCITY) == (1, 2)
    assert "#define MSCKF_FIX_POSITION 1" in hdr and "#define MSCKF_FIX_VELOCITY 2" in hdr
