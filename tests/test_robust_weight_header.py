"""The robust loss of csrc/robust_weight.h (the formula k_robust and the C ABI share) through a stand-alone driver built with
the host compiler from the header alone, under AddressSanitizer and UBSan: phi at s = 0, just below / at / just above k, huge,
inf and NaN for both losses against the Python formula of tests/robust_ref.py, and the parameter check at its boundaries."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import robust_ref as rr
from conftest import ROOT

HEADER_DIR = os.path.join(ROOT, "monocular-visual-inertial-msckf_amd", "csrc")

DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include "robust_weight.h"
static void show(const char* name, double x) { std::uint64_t b; std::memcpy(&b, &x, 8); std::printf("%s %016llx\n", name, (unsigned long long)b); }
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double ks[2] = {1.345, 2.385};
    for (int loss = 1; loss <= 2; ++loss) {
        const double k = ks[loss - 1], w_min = 0.05;
        const double s[8] = {0.0, std::nextafter(k, 0.0), k, std::nextafter(k, 4.0), 3.0 * k, 1e300, inf, nan};
        const char* tag[8] = {"zero", "below", "at", "above", "three", "huge", "inf", "nan"};
        for (int i = 0; i < 8; ++i) {
            char name[32];
            std::snprintf(name, sizeof name, "phi%d_%s", loss, tag[i]);
            show(name, robust_phi(loss, k, w_min, s[i]));
        }
        char name[32];
        std::snprintf(name, sizeof name, "phi%d_floor1", loss);
        show(name, robust_phi(loss, k, 1.0, 3.0 * k));            // w_min = 1: no view is down-weighted
    }
    show("phi0_three", robust_phi(0, 1.345, 0.05, 4.0));         // the loss off
    auto ok = [](const char* name, int loss, int reserved, double k, double w_min) {
        std::printf("%s %016llx\n", name, (unsigned long long)robust_params_ok(loss, reserved, k, w_min));
    };
    ok("ok_off", 0, 0, 1.345, 0.05); ok("ok_huber", 1, 0, 1.345, 0.05); ok("ok_cauchy", 2, 0, 2.385, 0.05);
    ok("bad_loss_m1", -1, 0, 1.345, 0.05); ok("bad_loss_3", 3, 0, 1.345, 0.05); ok("bad_reserved", 1, 1, 1.345, 0.05);
    ok("bad_k_zero", 1, 0, 0.0, 0.05); ok("bad_k_neg", 1, 0, -1.0, 0.05); ok("bad_k_inf", 1, 0, inf, 0.05); ok("bad_k_nan", 1, 0, nan, 0.05);
    ok("ok_k_tiny", 1, 0, std::numeric_limits<double>::denorm_min(), 0.05); ok("ok_k_max", 1, 0, std::numeric_limits<double>::max(), 0.05);
    ok("bad_w_zero", 1, 0, 1.345, 0.0); ok("bad_w_neg", 1, 0, 1.345, -0.05); ok("bad_w_above", 1, 0, 1.345, std::nextafter(1.0, 2.0));
    ok("bad_w_nan", 1, 0, 1.345, nan); ok("bad_w_inf", 1, 0, 1.345, inf);
    ok("ok_w_one", 1, 0, 1.345, 1.0); ok("ok_w_tiny", 1, 0, 1.345, std::numeric_limits<double>::denorm_min());
    return 0;
}
"""

PARAMS = {"ok_off": 1, "ok_huber": 1, "ok_cauchy": 1, "bad_loss_m1": 0, "bad_loss_3": 0, "bad_reserved": 0, "bad_k_zero": 0,
          "bad_k_neg": 0, "bad_k_inf": 0, "bad_k_nan": 0, "ok_k_tiny": 1, "ok_k_max": 1, "bad_w_zero": 0, "bad_w_neg": 0,
          "bad_w_above": 0, "bad_w_nan": 0, "bad_w_inf": 0, "ok_w_one": 1, "ok_w_tiny": 1}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("robust_weight")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", HEADER_DIR, "-o", exe, src], check=True, timeout=120)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    return {k: int(v, 16) for k, v in (line.split() for line in out.splitlines())}


def _f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_phi_against_the_python_formula(driver):
    for li, loss in ((1, "huber"), (2, "cauchy")):
        k = rr.LOSSES[loss]
        s = {"zero": 0.0, "below": math.nextafter(k, 0.0), "at": k, "above": math.nextafter(k, 4.0), "three": 3.0 * k,
             "huge": 1e300, "inf": math.inf, "nan": math.nan}
        for tag, sv in s.items():
            got, ref = _f(driver[f"phi{li}_{tag}"]), float(rr.phi(loss, k, rr.W_MIN, sv))
            # (one division, one square root, correctly rounded on both sides; Cauchy's square may be fused or not)
            assert abs(got - ref) <= 4e-16 * ref, (loss, tag, got, ref)
        assert _f(driver[f"phi{li}_zero"]) == 1.0
        assert _f(driver[f"phi{li}_huge"]) == rr.W_MIN                       # the floor
        assert _f(driver[f"phi{li}_inf"]) == 1.0 and _f(driver[f"phi{li}_nan"]) == 1.0
        assert _f(driver[f"phi{li}_floor1"]) == 1.0
    # Huber is EXACTLY 1 up to and at k, and below 1 or equal to it one ulp above (sqrt(1 - 2^-53) rounds to 1 - 2^-53)
    assert _f(driver["phi1_below"]) == 1.0 and _f(driver["phi1_at"]) == 1.0
    assert _f(driver["phi1_above"]) <= 1.0
    assert _f(driver["phi1_three"]) == float(np.sqrt(np.float64(1.345) / (3.0 * np.float64(1.345))))
    assert _f(driver["phi2_at"]) == float(np.sqrt(0.5))
    assert _f(driver["phi0_three"]) == 1.0


def test_parameter_check_at_its_boundaries(driver):
    assert {k: driver[k] for k in PARAMS} == PARAMS


def test_header_and_abi_agree():
    hdr = open(os.path.join(ROOT, "include", "msckf_mi355x.h")).read()
    for name, val in (("OFF", 0), ("HUBER", 1), ("CAUCHY", 2)):
        assert f"#define MSCKF_ROBUST_{name} {val}" in hdr
    assert "constexpr int kRobustOff = 0, kRobustHuber = 1, kRobustCauchy = 2;" in open(os.path.join(HEADER_DIR, "robust_weight.h")).read()
    from msckf_amd import _ffi
    assert (_ffi.ROBUST_OFF, _ffi.ROBUST_HUBER, _ffi.ROBUST_CAUCHY) == (0, 1, 2)
    import ctypes
    assert ctypes.sizeof(_ffi.RobustParamsC) == 24
    assert "msckf_set_robust" in _ffi.SYMBOLS and "msckf_get_view_weights" in _ffi.SYMBOLS
