"""The match's search window and distinctiveness margin, the host side: the rule restated in `match_options_ref.py`.

a  With radius = +inf and margin = 0 the rule gives `match_ref.match`'s pairs on every frame of the reference's fixture.
b  The case set the GPU tests run (`match_options_ref.SHAPES`: the tails of the 16-wide tiles on both operands and both lane
   shares of D) passes `guards()` under every mode, and every reason code 0..4 occurs at least twice over it.
c  The aliasing property on the committed seeds: the plain rule yields wrong pairs and loses a fifth of the true ones; the
   rule with the window yields no wrong pair and at least the plain rule's true pairs.
d  The declarations: header, `_ffi.SYMBOLS`, the options struct."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT
import match_options_ref as mo
import match_ref

INF = float("inf")


@pytest.fixture(scope="module")
def cases():
    return {shape: mo.case(*shape) for shape in mo.SHAPES}


# ---- a ---------------------------------------------------------------------------------------------------------------------
def test_an_infinite_window_and_no_margin_is_the_plain_rule_on_the_fixture():
    fx = match_ref.Fixture()
    min_cos = float(fx.z["params"][0])
    rng = np.random.default_rng(0)
    checked = pairs = 0
    for f in range(1, fx.n_frames):
        A, fr = fx.frame(f - 1)["out_table"], fx.frame(f)
        if len(A) == 0:
            continue
        idx1, idx2, _ = match_ref.match(A, fr["desc"], min_cos)
        m = mo.match(A, fr["desc"], min_cos, rng.uniform(0, 600, (len(A), 2)), fr["kp"], INF, 0.0)
        assert np.array_equal(m.idx1, idx1) and np.array_equal(m.idx2, idx2), f
        off = mo.match(A, fr["desc"], min_cos)                          # both options off: no keypoints needed
        assert np.array_equal(off.idx1, idx1) and np.array_equal(off.why, m.why)
        assert set(m.why.tolist()) <= {0, 2, 3}
        if not fr["skipped"]:
            assert np.array_equal(np.column_stack([m.idx1, m.idx2]), fr["pairs"]), f
        checked += 1
        pairs += len(idx1)
    assert checked >= 9 and pairs > 0


# ---- b ---------------------------------------------------------------------------------------------------------------------
def test_the_case_set_is_guarded_and_reaches_every_reason_code(cases):
    assert sorted(cases) == sorted(mo.SHAPES) and {(T % 16, n % 16) for T, n, _ in mo.SHAPES} >= {(1, 1), (15, 0), (0, 1), (1, 8)}
    seen = {name: Counter() for name in mo.MODES}
    for (T, n, D), c in cases.items():
        assert c["A"].shape == (T, D) and c["B"].shape == (n, D) and c["A"].dtype == c["B"].dtype == np.float32
        for name, (radius, margin) in mo.MODES.items():
            m = mo.guards(c["A"], c["B"], mo.MIN_COS, c["uvA"], c["uvB"], radius, margin)
            seen[name].update(m.why.tolist())
    print({k: dict(v) for k, v in seen.items()})
    assert all(seen["both"][code] >= 2 for code in range(5)), seen["both"]
    assert seen["margin"][1] == 0 and seen["window"][4] == 0            # a code belongs to its option
    assert all(seen["window"][code] >= 2 for code in (0, 1, 2, 3)) and all(seen["margin"][code] >= 2 for code in (0, 2, 3, 4))


def test_the_guards_refuse_what_rounding_could_decide():
    A = np.array([[1.0, 0.0], [0.0, 1.0]], dtype=np.float32)
    uvA = np.array([[100.0, 100.0], [300.0, 100.0]])
    B = np.array([[0.9, 0.0], [0.9 - 5e-5, 0.0], [0.0, 0.9]], dtype=np.float32)
    uvB = np.array([[101.0, 100.0], [102.0, 100.0], [301.0, 100.0]])
    with pytest.raises(AssertionError, match="runner-up"):
        mo.guards(A, B, 0.5, uvA, uvB, 20.0, 0.0)
    B[1, 0] = 0.8
    mo.guards(A, B, 0.5, uvA, uvB, 20.0, 0.0)
    with pytest.raises(AssertionError, match="threshold"):
        mo.guards(A, B, 0.9 + 5e-5, uvA, uvB, 20.0, 0.0)
    with pytest.raises(AssertionError, match="margin"):
        mo.guards(A, B, 0.5, uvA, uvB, 20.0, 0.1 + 5e-5)
    with pytest.raises(AssertionError, match="radius"):
        mo.guards(A, B, 0.5, uvA, uvB, 2.0 + 5e-7, 0.0)


def test_ties_second_bests_and_none():
    A = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], dtype=np.float32)
    uvA = np.array([[0.0, 0.0], [100.0, 0.0], [500.0, 0.0]])
    B = np.array([[2.0, 0.0], [2.0, 0.0], [0.0, 3.0]], dtype=np.float32)
    uvB = np.array([[3.0, 4.0], [0.0, 5.0], [100.0, 1.0]])
    m = mo.match(A, B, 0.5, uvA, uvB, 5.0, 0.0)                         # distance 5 is inside (<=)
    assert m.m12.tolist() == [0, 2, -1] and m.s1.tolist() == [2.0, 3.0, -INF] and m.s2.tolist() == [2.0, -INF, -INF]
    assert m.m21.tolist() == [0, 0, 1] and m.c2.tolist() == [-INF, -INF, -INF]
    assert m.why.tolist() == [0, 0, 1] and m.idx2.tolist() == [0, 2]
    m = mo.match(A, B, 0.5, uvA, uvB, 5.0, 0.25)                        # equal bests: a margin of 0 between them
    assert m.why.tolist() == [4, 0, 1]
    m = mo.match(A, B, 0.5, uvA, uvB, 4.99, 0.0)
    assert m.why.tolist() == [1, 0, 1]
    m = mo.match(A, B, 3.0, uvA, uvB, INF, 0.0)                         # the threshold is strict; row 2 loses to row 0
    assert m.why.tolist() == [3, 3, 2]


# ---- c ---------------------------------------------------------------------------------------------------------------------
def test_the_window_removes_the_aliasing_of_the_plain_rule(cases):
    shown = 0
    for (T, n, D), c in cases.items():
        if T < 8:
            continue
        true = len(c["true"])
        idx1, idx2, _ = match_ref.match(c["A"], c["B"], mo.MIN_COS)
        plain_true, plain_wrong = mo.score(c, idx1, idx2)
        w = mo.match(c["A"], c["B"], mo.MIN_COS, c["uvA"], c["uvB"], mo.RADIUS, 0.0)
        win_true, win_wrong = mo.score(c, w.idx1, w.idx2)
        print(f"T / n / D {T} / {n} / {D}: pairs plain {len(idx1)}, window {len(w.idx1)}; wrong {plain_wrong}, {win_wrong}; true pairs {true}")
        assert plain_wrong >= 1 and 5 * (true - plain_true) >= true
        assert win_wrong == 0 and win_true >= plain_true and win_true == true
        shown += 1
    assert shown == 5


def test_the_store_follows_the_last_keypoint():
    """The wrapper of `match_ref.Store`: the window's centre is the appended keypoint, and behind a removed clone the last
    view that is left."""
    Kmat = np.array([[400.0, 0.0, 320.0], [0.0, 400.0, 240.0], [0.0, 0.0, 1.0]])
    st = mo.Store(Kmat, 0.5, INF, INF, radius=20.0)
    d = np.eye(8, dtype=np.float32)[:2]
    p0 = np.array([[100.0, 100.0], [300.0, 200.0]])
    for key in range(3):
        st.add_camera(key, np.eye(3), [0.2 * key, 0.0, 0.0])
    ids, res, _ = st.intake(0, p0, d, [1.0, 1.0])
    assert res.tolist() == [4, 4] and st.last is None
    ids, res, _ = st.intake(1, p0 + [15.0, 0.0], d, [1.0, 1.0])
    assert ids.tolist() == [1, 2] and res.tolist() == [0, 0] and np.array_equal(st.centres(), p0 + [15.0, 0.0])
    assert st.intake(2, p0 - [15.0, 0.0], d, [1.0, 1.0]) is None and st.last.why.tolist() == [1, 1]   # 30 px from the centres
    st.remove_cameras([1])
    assert np.array_equal(st.centres(), p0)
    ids, res, _ = st.intake(2, p0 - [15.0, 0.0], d, [1.0, 1.0])
    assert ids.tolist() == [1, 2] and res.tolist() == [0, 0] and st.last.why.tolist() == [0, 0]


# ---- d ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_ffi_binds_them(engine_lib):
    from msckf_amd import _ffi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msckf_mi355x.h")).read(), flags=re.S)
    txt = re.sub(r"\s+([,)])", r"\1", re.sub(r"\s+", " ", txt))
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    want = {
        "msckf_tracks_set_match_options": (r"msckf_ctx\* ctx, const msckf_match_options\* options", [vp, C.POINTER(_ffi.MatchOptionsC)]),
        "msckf_tracks_match_at": (r"msckf_ctx\* ctx, double \w+, int32_t \w+, int32_t n, const float\* desc, const double\* uv,"
                                  r" int32_t\* track_id_out, float\* sim_out", [vp, f64, i32, i32, vp, vp, vp, vp]),
        "msckf_tracks_match_report": (r"msckf_ctx\* ctx, int32_t\* T_out, int32_t\* ids_out, uint8_t\* why_out, int32_t cap", [vp, vp, vp, vp, i32]),
    }
    for name, (proto, argtypes) in want.items():
        assert re.search(r"\bint " + name + r"\(" + proto + r"\);", txt), name
        assert name in _ffi.SYMBOLS
        fn = getattr(engine_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    body = re.search(r"typedef struct msckf_match_options \{(.*?)\} msckf_match_options;", txt).group(1)
    assert re.findall(r"double (\w+);", body) == [n for n, _ in _ffi.MatchOptionsC._fields_] and C.sizeof(_ffi.MatchOptionsC) == 16
    assert _ffi.ABI_VERSION == 2 and re.search(r"#define MSCKF_ABI_VERSION 2\b", txt)
