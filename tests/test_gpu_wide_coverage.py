"""`k_feature_wide`, the second pass of `k_gather` and the 64-view slot map of `k_fold` / `k_fold_g` at every track length 32 .. 64,
on slot layouts other than consecutive views of a window of at most 64 clones, and on the camera geometries of
tests/geometry_cases.py.  The yardstick is `oracle.update`; the batches, what each is for and the conditions
the oracle alone meets on them are in tests/wide_geometry_cases.py and tests/test_wide_coverage.py.

Tolerances, those of tests/test_gpu_wide_tracks.py: dx and P+ 1e-8 relative, gamma 1e-8 relative (atol 1e-12), mask and rejected
count equal, P+ bit-symmetric; through `debug_gate` / `debug_compressed`: the row count 2M - rank per track against
`geometry_cases.kernel_qr`, T^T T = H^T H and T^T r_n = H^T r at 1e-8.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import filter_prior as fp
import geometry_cases as gc
import wide_cases as wc
import wide_geometry_cases as wg
from conftest import load_golden, rel_err
from msckf_amd import _ffi
from test_gpu_wide_tracks import GAMMA_TOL, TOL, _code, _engine, _hold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_221():
    e = _engine(max_clones=221)
    yield e
    e.close()


_RANKS = {}


def _ranks(key, prob):
    """K2's rank per track by its NumPy restatement."""
    if key not in _RANKS:
        _RANKS[key] = np.array([t[0].rank for t in gc.track_table(prob)])
    return _RANKS[key]


def _debug(e, key, what, prob, ref):
    """Rows per track, the compressed system, the gate bytes; no track split, the merge tree."""
    gam, q = e.debug_gate()
    rows = 2 * wc.views(prob) - _ranks(key, prob)
    print(f"{what}: rows per track {q.tolist()}", flush=True)
    assert np.array_equal(q, rows), (what, q, rows)
    T, rn = e.debug_compressed()
    H, r = ref["H_X"][:, 15:], ref["r_o"]
    e_T, e_r = rel_err(T.T @ T, H.T @ H), rel_err(T.T @ rn, H.T @ r)
    print(f"{what}: compressed system T^T T {e_T:.2e}, T^T r_n {e_r:.2e}", flush=True)
    assert e_T < TOL and e_r < TOL, (what, e_T, e_r)
    codes, block_codes, _ = e.gate_codes()
    assert np.array_equal(codes, ref["accepted"]) and len(block_codes) == 0, what
    s = e.debug_split()
    assert s["long_tracks"] == 0 and s["band_plan"] == 0, (what, s)
    return gam


def _both_paths(e, key, prob, ref):
    """The one-shot call and load / run / result, each against the oracle and bit-equal to each other."""
    res = e.update_problem(prob)
    gam = e.debug_gate()[0]
    err = np.abs(gam - ref["gamma"]) / np.abs(ref["gamma"])
    print(f"{key}: gamma relative error per track (views: error) " + " ".join(f"{m}:{x:.1e}" for m, x in zip(wc.views(prob), err)), flush=True)
    _hold(res, ref, f"{key} update_problem", gam)
    assert res.stats["stacked_rows"] == ref["H_X"].shape[0]
    _debug(e, key, f"{key} update_problem", prob, ref)
    e.load(prob)
    e.run()
    res2 = e.result()
    _hold(res2, ref, f"{key} load/run/result", e.debug_gate()[0])
    _debug(e, key, f"{key} load/run/result", prob, ref)
    assert np.array_equal(res.dx, res2.dx) and np.array_equal(res.P_new, res2.P_new) and np.array_equal(res.accepted, res2.accepted)
    assert np.array_equal(gam, e.debug_gate()[0])
    return res, gam


# ---- A: every length ---------------------------------------------------------------------------------------------------------

def test_every_length_32_to_64(eng):
    prob, ref = wg.all_lengths()
    _both_paths(eng, "all_lengths", prob, ref)


def test_every_length_at_rank_two(eng):
    prob, ref = wg.all_lengths_rank2()
    _both_paths(eng, "all_lengths_rank2", prob, ref)
    assert {64, 96, 112, 126} <= set(eng.debug_gate()[1].tolist())


# ---- B: slot layouts ------------------------------------------------------------------------------------------------------------

def test_views_that_skip_clones(eng):
    prob, ref = wg.holes_64()
    _both_paths(eng, "holes_64", prob, ref)


def test_views_in_a_shuffled_order(eng):
    """Against the oracle on the shuffled batch, and against the engine's own result on the ascending one."""
    base, base_ref = wg.holes_64()
    res0 = eng.update_problem(base)
    gam0 = eng.debug_gate()[0]
    prob, ref = wg.shuffled()
    res, gam = _both_paths(eng, "shuffled", prob, ref)
    e_dx, e_P = rel_err(res.dx, res0.dx), rel_err(res.P_new, res0.P_new)
    e_g = float(np.max(np.abs(gam - gam0) / np.abs(gam0)))
    print(f"shuffled against holes_64 on the engine: dx {e_dx:.2e} P+ {e_P:.2e} gamma {e_g:.2e}", flush=True)
    assert np.array_equal(res.accepted, res0.accepted) and res.n_rejected == res0.n_rejected
    assert e_dx < TOL and e_P < TOL
    np.testing.assert_allclose(gam, gam0, **GAMMA_TOL)


@pytest.mark.parametrize("N", list(wg.BEYOND))
def test_windows_beyond_64_clones(eng_221, N):
    prob, ref = wg.beyond_64(N)
    _both_paths(eng_221, f"beyond_{N}", prob, ref)


def test_refusals_on_a_wide_context(eng_221):
    first, first_ref = wc.synth_case("first")

    def still_good(what):
        res = eng_221.update_problem(first)
        _hold(res, first_ref, what, eng_221.debug_gate()[0])

    for N, (prob, _) in ((64, wg.holes_64()), (65, wg.beyond_64(65))):       # the `seen` bitmask, and the general check
        j = int(np.argmax(wc.views(prob)))
        dup = wg.with_duplicate_slot(prob, j, 3, int(wc.views(prob)[j]) - 2)
        code = _code(eng_221.update_problem, dup)
        print(f"duplicate slot at N = {N}: code {code}", flush=True)
        assert code == _ffi.ERR_DUP_SLOT
        still_good(f"after a duplicate slot at N = {N}")
    prob, _ = wg.beyond_64(65)
    code = _code(eng_221.update_problem, wg.with_slot(prob, 0, 40, 65))
    print(f"slot N: code {code}", flush=True)
    assert code == _ffi.ERR_ARG
    still_good("after a slot equal to N")


def test_wide_narrow_wide_on_one_context():
    """Nothing of a wide batch (the list of wide tracks, the narrow kernels' longest track, the plan) outlives it."""
    wide, ref = wg.holes_64()
    narrow, z = load_golden("cfg2_A")
    with _engine(max_features=512) as fresh:
        want = fresh.update_problem(narrow)
        want_split = fresh.debug_split()
    with _engine(max_features=512) as e:
        a = e.update_problem(wide)
        gam_a = e.debug_gate()[0]
        _hold(a, ref, "wide, first", gam_a)
        n = e.update_problem(narrow)
        assert e.debug_split() == want_split
        b = e.update_problem(wide)
        gam_b = e.debug_gate()[0]
        _hold(b, ref, "wide, second", gam_b)
    print(f"narrow between two wide batches: dx {rel_err(n.dx, z['dx']):.2e} P+ {rel_err(n.P_new, z['P_new']):.2e}", flush=True)
    assert n.status == want.status == int(z["status"]) and np.array_equal(n.accepted, z["accepted"])
    assert np.array_equal(n.dx, want.dx) and np.array_equal(n.P_new, want.P_new) and np.array_equal(n.accepted, want.accepted)
    assert rel_err(n.dx, z["dx"]) < TOL and rel_err(n.P_new, z["P_new"]) < TOL
    assert np.array_equal(a.dx, b.dx) and np.array_equal(a.P_new, b.P_new) and np.array_equal(a.accepted, b.accepted)
    assert np.array_equal(gam_a, gam_b)


# ---- C: geometry families -------------------------------------------------------------------------------------------------------

def _check_result(name, what, res, prob, ref):
    """tests/test_gpu_geometry.py's check_result: the five measures of `filter_prior.metrics`."""
    m = fp.metrics(res.dx, res.P_new, ref, prob.P)
    print(f"WIDEGEOMETRYGPU {name} {what} " + " ".join(f"{x:.2e}" for x in m), flush=True)
    assert res.status == ref["status"] == 0, (name, what)
    assert np.array_equal(res.accepted, ref["accepted"]), (name, what)
    assert res.stats["not_spd"] == 0 and res.stats["n_accepted"] == int(ref["accepted"].sum()), (name, what, res.stats)
    assert np.array_equal(res.P_new, res.P_new.T), (name, what)
    assert max(m) < TOL, (name, what, m)


def _check_debug(e, name, what, prob, ref):
    """tests/test_gpu_geometry.py's check_debug, with the rank per track from kernel_qr."""
    gam, q = e.debug_gate()
    want_rank = 2 if wg.GEOMETRY[name].exact_rank2 else 3
    ranks = _ranks(name, prob)
    err = float(np.max(np.abs(gam - ref["gamma"]) / np.abs(ref["gamma"])))
    print(f"WIDEGEOMETRYGPU {name} {what} gamma {err:.2e} rows {q.tolist()}", flush=True)
    assert np.all(ranks == want_rank) and np.array_equal(q, 2 * wc.views(prob) - ranks), (name, what, q)
    np.testing.assert_allclose(gam, ref["gamma"], **GAMMA_TOL)
    _debug(e, name, f"WIDEGEOMETRYGPU {name} {what}", prob, ref)


@pytest.mark.parametrize("name", list(wg.GEOMETRY))
def test_geometry_families_at_wide_lengths(eng, name):
    prob, ref = wg.geometry(name)
    res = eng.update_problem(prob)
    _check_result(name, "one-shot", res, prob, ref)
    _check_debug(eng, name, "one-shot", prob, ref)
    assert res.stats["stacked_rows"] == ref["H_X"].shape[0]
    eng.load(prob)
    eng.run()
    res2 = eng.result()
    _check_result(name, "resident", res2, prob, ref)
    _check_debug(eng, name, "resident", prob, ref)
    assert np.array_equal(res2.dx, res.dx) and np.array_equal(res2.P_new, res.P_new), name
