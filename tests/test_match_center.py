"""The centre of the match's search window, the host side: the rule of `csrc/match_center.h` restated in
`match_center_ref.py`.

a  The header alone, through a stand-alone driver built with the host compiler under AddressSanitizer and UBSan, over the
   case set (600 cases: bearings and points in front of, grazing and behind the newest clone, both modes, triangulated or
   not, rho positive, zero and negative, two intrinsics): `how` equal, the centres within the bound of b.
b  The tolerance.  The truth is the restatement in `np.longdouble` (eps 1.08e-19 < 2e-19: the x87 format).  e64 is the worst
   error in pixels of the fp64 restatement against it over the cases fit for the bound (h_z >= 0.2 |c|, |rho (base - t_n)|
   <= 10; 406 of the 600), and the bound is 8 x e64: room for a compiler that contracts or reorders the same ~40 flops.
   Measured (x86-64, no FMA): e64 = 7.02e-13 px at centres of up to 2287 px, so the bound is 5.62e-12 px.  The header is held
   to it against the truth.  Every case anywhere has |h_z| >= 1e-3 |c| for every projection the rule may evaluate, so `how`
   cannot depend on rounding.  The header is also compiled for gfx950 inside a one-lane-per-case probe kernel (compiled, not
   run: no kernel of the engine calls it yet) and must need neither scratch nor LDS there.
c  The scenes, with the restatement alone.  Yaw sweep (4 degrees and 0.05 m per frame, depths 8-12 m, radius 12 px, six
   frames): centred on the last keypoint no track has a keypoint inside its window (closest 14.4 px); centred by ROTATED
   every track whose point projects into the image pairs with its own keypoint (within 3.4 px of the centre).  Lateral step
   (0.4 m per frame, depths 4-5 m): at frame 2 ROTATED finds nothing (closest 14.1 px), POINT with exact points pairs
   every visible track.  Every track-keypoint distance is at least GUARD_PX away from the radius.  A track without a centre
   goes through the window's rule as NaN (`NaN <= r^2` is false), not as a far point."""
import os
import subprocess

import numpy as np
import pytest

import match_center_ref as mc
from conftest import ROOT

INF = float("inf")
HEADER_DIR = os.path.join(ROOT, "monocular-visual-inertial-msckf_amd", "csrc")

# input: int32 n; int32 mode[n], tri[n]; double Rn[9 n], tn[3 n], K[9 n], d[3 n], base[3 n], m[3 n], rho[n]
# output: one line per case: how, u, v (the doubles as hex words)
DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "match_center.h"
template <typename T> static std::vector<T> take(std::FILE* f, std::size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const std::size_t n = take<std::int32_t>(f, 1)[0];
    const std::vector<std::int32_t> mode = take<std::int32_t>(f, n), tri = take<std::int32_t>(f, n);
    const std::vector<double> Rn = take<double>(f, 9 * n), tn = take<double>(f, 3 * n), K = take<double>(f, 9 * n), d = take<double>(f, 3 * n),
                              base = take<double>(f, 3 * n), m = take<double>(f, 3 * n), rho = take<double>(f, n);
    std::fclose(f);
    for (std::size_t i = 0; i < n; ++i) {
        double uv[2] = {0.0, 0.0};
        const int how = msckf::match_center(mode[i], &Rn[9 * i], &tn[3 * i], &K[9 * i], &d[3 * i], &base[3 * i], &m[3 * i], rho[i],
                                            tri[i] != 0, uv);
        std::uint64_t b[2];
        std::memcpy(b, uv, 16);
        std::printf("%d %016llx %016llx\n", how, (unsigned long long)b[0], (unsigned long long)b[1]);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def cases():
    cs = mc.case_set()
    truth, how = mc.evaluate(cs, np.longdouble)
    return cs, truth, how


def tolerance(cs, truth):
    """(e64, the bound): b of the docstring."""
    got, _ = mc.evaluate(cs, np.float64)
    e64 = mc.pixel_error(got[cs["bound"]], truth[cs["bound"]])
    return e64, 8 * e64


# ---- a, b -------------------------------------------------------------------------------------------------------------------
def test_the_case_set_covers_the_rule(cases):
    cs, truth, how = cases
    assert np.finfo(np.longdouble).eps < 2e-19
    n = len(how)
    for i in range(n):
        fit, bound = mc.conditions(int(cs["mode"][i]), cs["Rn"][i], cs["tn"][i], cs["K"][i], cs["d"][i], cs["base"][i], cs["m"][i],
                                   cs["rho"][i], bool(cs["tri"][i]))
        assert fit and bound == bool(cs["bound"][i]), i
    point = cs["mode"] == mc.POINT
    assert {(int(m), int(h)) for m, h in zip(cs["mode"], how)} == {(1, 1), (1, 3), (2, 1), (2, 2), (2, 3)}
    assert (how[point & (cs["tri"] == 0)] != mc.HOW_POINT).all() and (point & (cs["tri"] == 0)).sum() >= 20
    assert (how[point & (cs["rho"] <= 0)] != mc.HOW_POINT).all() and (point & (cs["rho"] < 0)).sum() >= 10 and (point & (cs["rho"] == 0)).sum() >= 5
    assert np.isnan(truth[how == mc.HOW_NONE].astype(np.float64)).all() and np.isfinite(truth[how != mc.HOW_NONE].astype(np.float64)).all()
    assert cs["bound"].sum() >= 300 and {int(h) for h in how[cs["bound"]]} == {1, 2}


def test_the_fp64_restatement_decides_as_the_truth_and_sets_the_bound(cases):
    cs, truth, how = cases
    got, how64 = mc.evaluate(cs, np.float64)
    assert np.array_equal(how64, how)
    e64, bound = tolerance(cs, truth)
    print(f"e64 {e64:.3e} px, bound {bound:.3e} px, largest centre {float(np.abs(truth[cs['bound']]).max()):.0f} px")
    assert 0 < e64 < 1e-10


def test_header_driver_under_sanitizers(cases, tmp_path):
    cs, truth, how = cases
    src, exe, path = (os.path.join(tmp_path, x) for x in ("driver.cpp", "driver", "in.bin"))
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", HEADER_DIR, "-o", exe, src], check=True, timeout=120)
    with open(path, "wb") as f:
        np.array([len(how)], dtype=np.int32).tofile(f)
        for k in ("mode", "tri"):
            np.ascontiguousarray(cs[k], dtype=np.int32).tofile(f)
        for k in ("Rn", "tn", "K", "d", "base", "m", "rho"):
            np.ascontiguousarray(cs[k], dtype=np.float64).tofile(f)
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True, timeout=30).stdout
    rows = [line.split() for line in out.splitlines()]
    assert len(rows) == len(how)
    got_how = np.array([int(r[0]) for r in rows], dtype=np.uint8)
    got = np.array([[int(r[1], 16), int(r[2], 16)] for r in rows], dtype=np.uint64).view(np.float64)
    assert np.array_equal(got_how, how)
    e64, bound = tolerance(cs, truth)
    err = mc.pixel_error(got[cs["bound"]], truth[cs["bound"]])
    print(f"header vs truth {err:.3e} px, bound {bound:.3e} px")
    assert err <= bound
    assert np.isnan(got[how == mc.HOW_NONE]).all() and np.isfinite(got[how != mc.HOW_NONE]).all()


PROBE = r"""
#include <hip/hip_runtime.h>
#include "match_center.h"
__global__ __launch_bounds__(256) void probe(int n, const int* mode, const int* tri, const double* Rn, const double* tn, const double* K,
                                             const double* d, const double* base, const double* m, const double* rho, double* uv, int* how) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double c[2];
    how[i] = msckf::match_center(mode[i], Rn + 9 * i, tn + 3 * i, K + 9 * i, d + 3 * i, base + 3 * i, m + 3 * i, rho[i], tri[i] != 0, c);
    uv[2 * i] = c[0];
    uv[2 * i + 1] = c[1];
}
"""


def test_header_compiles_for_the_device_without_scratch(tmp_path):
    """The flags of `csrc/Makefile`, device code only; nothing is run."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src, obj = os.path.join(tmp_path, "probe.hip"), os.path.join(tmp_path, "probe.s")
    with open(src, "w") as f:
        f.write(PROBE)
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-ffp-contract=on", "-S", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", HEADER_DIR, "-o", obj, src], check=True, capture_output=True, text=True,
                         timeout=300).stderr
    assert "Function Name: _Z5probe" in out
    for key in ("ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "VGPRs Spill", "SGPRs Spill"):
        assert key + ": 0" in out, (key, out)
    assert "Dynamic Stack: False" in out


# ---- c -------------------------------------------------------------------------------------------------------------------
def _own(store, ids, scene, who):
    """(T, n) bool: keypoint j of the frame is the point table track i was created from."""
    first = scene["frames"][0][0]
    return np.array([[first[t - 1] == w for w in who] for t in ids], dtype=bool).reshape(len(ids), len(who))


def sweep(scene, mode, after_frame=None):
    """The yaw sweep on the model under `mode`, the tracks a frame did not match removed behind it.  Per frame k >= 1:
    (table ids, window distances from the last keypoints, from the centres, `own`, what the intake returned)."""
    st = mc.Store(mc.K, mc.MIN_COS, INF, INF, radius=mc.RADIUS, mode=mode)
    log = []
    for k, (who, kp, d) in enumerate(scene["frames"]):
        st.add_camera(k, *scene["poses"][k])
        ids = list(st.table_ids)
        if k > 0:
            last = np.array([st.tracks[t].uv[-1] for t in ids])
            entry = [ids, mc.window_distances(last, kp), mc.window_distances(st.centres(), kp), _own(st, ids, scene, who)]
        out = st.intake(k, kp, d, np.ones(len(d)))                   # (guarded: every distance GUARD_PX from the radius)
        if k > 0:
            log.append(entry + [out])
        if out is not None:
            st.remove_tracks([t for t in list(st.tracks) if st.tracks[t].lost > 0])
        if after_frame:
            after_frame(k, st, out)
    return st, log


def test_yaw_sweep_last_finds_nothing_rotated_finds_every_track():
    scene = mc.yaw_sweep()
    closest, furthest = INF, 0.0
    st, log = sweep(scene, "rotated")
    assert len(log) == mc.YAW_FRAMES
    for k, (ids, d_last, d_rot, own, out) in enumerate(log, start=1):
        who = scene["frames"][k][0]
        assert (d_last > mc.RADIUS + mc.GUARD_PX).all(), k            # LAST: no keypoint in any window
        closest = min(closest, float(d_last.min()))
        assert (own.sum(axis=0) == 1).all() and len(who) >= 50, k     # every keypoint is a live track's point
        assert np.array_equal(d_rot <= mc.RADIUS, own), k             # ROTATED: its own keypoint, and no other
        furthest = max(furthest, float(d_rot[own].max()))
        got_ids, res, pairs = out
        assert (res == 0).all() and len(pairs) == len(who), k
        first = scene["frames"][0][0]
        assert [int(first[t - 1]) for t in got_ids] == who.tolist(), k
    print(f"LAST: closest keypoint {closest:.2f} px; ROTATED: own keypoint within {furthest:.2f} px")
    assert len(st.tracks) == len(scene["frames"][-1][0])
    # the same frames under LAST on the model: every frame is skipped
    plain = mc.Store(mc.K, mc.MIN_COS, INF, INF, radius=mc.RADIUS, mode="last", guarded=False)
    for k, (who, kp, d) in enumerate(scene["frames"]):
        plain.add_camera(k, *scene["poses"][k])
        out = plain.intake(k, kp, d, np.ones(len(d)))
        assert (out is None) == (k > 0), k


def test_lateral_step_rotated_finds_nothing_point_finds_every_track():
    scene = mc.lateral_step()
    first = scene["frames"][0][0]
    shown = {}
    for mode in ("rotated", "point"):
        st = mc.Store(mc.K, mc.MIN_COS, INF, INF, radius=0.0, mode=mode)
        for k in (0, 1):                                              # the radius off: the plain rule
            st.add_camera(k, *scene["poses"][k])
            who, kp, d = scene["frames"][k]
            out = st.intake(k, kp, d, np.ones(len(d)))
            assert (out[1] == (4 if k == 0 else 0)).all()
        for t in st.tracks:
            st.points[t] = mc.exact_point(scene["W"][first[t - 1]], scene["poses"][0][1])
        st.radius = mc.RADIUS
        st.add_camera(2, *scene["poses"][2])
        who, kp, d = scene["frames"][2]
        ids = list(st.table_ids)
        centres, how = st.centres_how()
        dist, own = mc.window_distances(centres, kp), _own(st, ids, scene, who)
        out = st.intake(2, kp, d, np.ones(len(d)))
        if mode == "rotated":
            assert (how == mc.HOW_ROTATED).all() and (dist > mc.RADIUS + mc.GUARD_PX).all()
            assert out is None and (st.last.why == 1).all()
            shown[mode] = float(dist.min())
        else:
            assert (how == mc.HOW_POINT).all() and np.array_equal(dist <= mc.RADIUS, own)
            assert len(who) < len(ids) and (own.sum(axis=0) == 1).all()          # some points left the image
            got_ids, res, pairs = out
            assert (res == 0).all() and [int(first[t - 1]) for t in got_ids] == who.tolist()
            assert (st.last.why[own.any(axis=1)] == 0).all() and (st.last.why[~own.any(axis=1)] == 1).all()
            shown[mode] = float(dist[own].max())
    print(f"ROTATED: closest keypoint {shown['rotated']:.2f} px; POINT: own keypoint within {shown['point']:.2e} px")


def test_the_store_model_falls_back_and_reports_none():
    """POINT without a point is ROTATED; a bearing behind the newest clone has no centre and no keypoint in its window."""
    st = mc.Store(mc.K, 0.5, INF, INF, radius=20.0, mode="point")
    d = np.eye(8, dtype=np.float32)[:2]
    p0 = np.array([[100.0, 100.0], [300.0, 200.0]])
    st.add_camera(0, np.eye(3), np.zeros(3))
    st.intake(0, p0, d, [1.0, 1.0])
    st.add_camera(1, mc.yaw(3.0), np.zeros(3))
    c, how = st.centres_how()
    assert how.tolist() == [1, 1] and (np.abs(c - p0)[:, 0] > 15).all()
    st.add_camera(2, mc.yaw(180.0), np.zeros(3))
    c, how = st.centres_how()
    assert how.tolist() == [3, 3] and np.isnan(c).all()
    assert st.intake(2, p0, d, [1.0, 1.0]) is None and st.last.why.tolist() == [1, 1]
