"""Tracks of 32 to 64 views (`MSCKF_MAX_TRACK_WIDE`) on the device: `k_feature_wide` for K1-K4, one block per track on the
merge tree behind it.  The yardstick is `oracle.update` (reference `MSCKF.py:570-614`, which takes any track
length: `:573-588`); the batches, their reasons and their gate margins are in tests/wide_cases.py and
tests/test_wide_tracks.py.

Tolerances, the project's parity tolerances for long tracks (tests/test_gpu_split.py): dx and P+ 1e-8 relative, gamma
1e-8 relative (atol 1e-12), mask and rejected count equal, P+ bit-symmetric.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import wide_cases as wc
from conftest import load_golden, rel_err
from msckf_amd import _ffi, synth
from oracle import msckf_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 1e-8
GAMMA_TOL = dict(rtol=1e-8, atol=1e-12)


def _engine(**kw):
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=64, max_features=64, max_track=64)
    args.update(kw)
    return UpdateEngine(**args)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _code(fn, *a):
    with pytest.raises(_ffi.EngineError) as ei:
        fn(*a)
    return ei.value.code


def _hold(res, ref, what, gamma=None):
    e_dx, e_P = rel_err(res.dx, ref["dx"]), rel_err(res.P_new, ref["P_new"])
    print(f"{what}: dx {e_dx:.2e} P+ {e_P:.2e} accepted {int(res.accepted.sum())} rejected {res.n_rejected} rows {res.stats['stacked_rows']}", flush=True)
    assert res.status == int(ref["status"]), what
    assert np.array_equal(res.accepted, ref["accepted"]), what
    assert res.n_rejected == int(ref["n_rejected"]), what
    assert e_dx < TOL and e_P < TOL, (what, e_dx, e_P)
    assert np.array_equal(res.P_new, res.P_new.T), what
    if gamma is not None:
        err = np.abs(gamma - ref["gamma"]) / np.maximum(np.abs(ref["gamma"]), 1e-300)
        print(f"{what}: gamma worst relative error {err.max():.2e}", flush=True)
        np.testing.assert_allclose(gamma, ref["gamma"], **GAMMA_TOL)


def _one_shot(eng, prob, ref, what):
    res = eng.update_problem(prob)
    gam, q = eng.debug_gate()
    _hold(res, ref, what, gam)
    if "H_X" in ref:
        assert res.stats["stacked_rows"] == ref["H_X"].shape[0], what
    return res, q


# ---- 1, 2: the first wide sizes and the cap ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["first", "cap"])
def test_wide_tracks_against_the_oracle(eng, name):
    prob, ref = wc.synth_case(name)
    res, q = _one_shot(eng, prob, ref, name)
    assert np.array_equal(q, 2 * wc.views(prob) - 3)                 # rank 3 on the corridor
    assert eng.debug_split()["band_plan"] == 0 and eng.debug_split()["long_tracks"] == 0      # one block per track, the merge tree
    T, rn = eng.debug_compressed()                                   # T^T T = H^T H, T^T r_n = H^T r
    H, r = ref["H_X"][:, 15:], ref["r_o"]
    e_T, e_r = rel_err(T.T @ T, H.T @ H), rel_err(T.T @ rn, H.T @ r)
    print(f"{name}: compressed system T^T T {e_T:.2e}, T^T r_n {e_r:.2e}", flush=True)
    assert e_T < 1e-10 and e_r < 1e-10


# ---- 3: wide tracks among narrow ones, through both entry points ---------------------------------------------------------------
def test_mixed_batch_through_both_paths(eng):
    prob, ref = wc.synth_case("mixed")
    res, _ = _one_shot(eng, prob, ref, "mixed update_problem")
    eng.load(prob)
    eng.run()
    res2 = eng.result()
    gam2, _ = eng.debug_gate()
    _hold(res2, ref, "mixed load/run/result", gam2)
    assert np.array_equal(res.dx, res2.dx) and np.array_equal(res.P_new, res2.P_new) and np.array_equal(res.accepted, res2.accepted)
    eng.commit_covariance()
    assert np.array_equal(eng.covariance(), res2.P_new)


# ---- 4: the reference's own outputs ------------------------------------------------------------------------------------------
def test_the_wide_fixture(eng):
    prob, z = wc.fixture()
    res = eng.update_problem(prob)
    gam, q = eng.debug_gate()
    _hold(res, z, "edge_wide_tracks", gam)
    w, acc = wc.wide(prob), z["accepted"].astype(bool)
    assert (w & acc).any() and (w & ~acc).any()
    codes, block_codes, _ = eng.gate_codes()
    assert np.array_equal(codes, z["accepted"]) and len(block_codes) == 0            # 1 accepted, 0 rejected by the gate; nothing split
    # the rejected tracks, the wide ones among them, contribute no rows
    assert res.stats["stacked_rows"] == int(q[acc].sum()) == int((2 * wc.views(prob) - 3)[acc].sum())
    assert res.stats["n_accepted"] == 16 and res.stats["n_rejected"] == 8 and res.stats["not_spd"] == 0


# ---- 5: rank 2 -------------------------------------------------------------------------------------------------------------------
def test_rank_two_under_pure_rotation(eng):
    prob, ref, rows = wc.rank2_case()
    res, q = _one_shot(eng, prob, ref, "rank 2")
    assert np.array_equal(q, rows) and np.array_equal(q, 2 * wc.views(prob) - 2)


# ---- 6: views out of slot order ---------------------------------------------------------------------------------------------------
def test_views_in_descending_slot_order(eng):
    prob, ref = wc.reversed_case()
    _one_shot(eng, prob, ref, "reversed")


# ---- 7: per-view noise -----------------------------------------------------------------------------------------------------------
def test_heterogeneous_view_sigma(eng):
    het, ref = wc.weighted_case()
    res = eng.update_problem(het)
    gam, _ = eng.debug_gate()
    _hold(res, ref, "per-view noise, update_problem", gam)
    plain, _ = wc.synth_case("first")
    eng.load(plain)
    eng.set_view_sigma(het.view_sigma)
    eng.run()
    res2 = eng.result()
    _hold(res2, ref, "per-view noise, load + set_view_sigma")
    assert np.array_equal(res.dx, res2.dx) and np.array_equal(res.P_new, res2.P_new)


# ---- 8: the selection in front --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine_iters", [0, 8])
def test_selection_in_front_of_the_update(eng, refine_iters):
    """Flags against oracle.select_features; the chained update against oracle.update on the valid tracks fed the device's
    own inverse-depth points (as tests/test_gpu_select_refine.py holds its batches)."""
    prob, tracks, params, sel_ref = wc.select_case(refine_iters)
    eng.load(prob)
    eng.set_tracks(tracks)
    eng.run_select(params, prob.K)
    sel = eng.selection()
    eng.run()
    res = eng.result()
    codes = eng.gate_codes()[0]
    eng.clear_selection()
    assert np.array_equal(sel.flags & 7, sel_ref["flags"] & 7)
    valid = np.nonzero(sel.flags & 1)[0]
    picked = (sel.flags & 1) > 0
    assert (wc.wide(prob) & picked).sum() == 2 and (wc.wide(prob) & ~picked).sum() == 2
    assert np.all(codes[~picked] == 3) and np.all(codes[picked] != 3)           # a wide track that is not selected: byte 3, no rows
    if refine_iters == 0:
        assert rel_err(sel.idp_rho[valid], sel_ref["idp_rho"][valid]) < TOL and rel_err(sel.idp_m[valid], sel_ref["idp_m"][valid]) < TOL
    else:
        kept = (sel.flags & 8) > 0
        print(f"selection: refined points kept on {int(kept.sum())} tracks, {int(kept[wc.wide(prob)].sum())} of them wide", flush=True)
        assert kept.any()
    chained = prob.take(valid)
    chained.idp_m, chained.idp_rho = sel.idp_m[valid], sel.idp_rho[valid]
    out = oracle.update(chained, dense_noise=False)
    m = wc.margin(out)
    print(f"selection, refine_iters {refine_iters}: {len(valid)} valid, chained gate margin {m:.3f}", flush=True)
    assert m >= wc.MIN_MARGIN
    e_dx, e_P = rel_err(res.dx, out["dx"]), rel_err(res.P_new, out["P_new"])
    print(f"selection, refine_iters {refine_iters}: dx {e_dx:.2e} P+ {e_P:.2e}", flush=True)
    assert res.status == out["status"] == 0 and res.n_rejected == out["n_rejected"]
    assert np.array_equal(res.accepted[valid], out["accepted"]) and not res.accepted[np.setdiff1d(np.arange(prob.F), valid)].any()
    assert e_dx < TOL and e_P < TOL
    assert np.array_equal(res.P_new, res.P_new.T)


# ---- 9: the not-SPD verdict -------------------------------------------------------------------------------------------------------
def test_not_spd_gate_matrices(eng):
    """The indefinite prior of tests/test_gpu_gate_not_spd.py on case "first".  Wide tracks that see the cut-off clone get gate
    byte 2 and are dropped in front of the chi-square test; the call answers as it does for narrow tracks (that file's
    test_bad_tracks_are_dropped_and_reported and test_every_track_bad_is_a_no_op): the update of the good tracks alone, and a
    no-op (status 1, the prior kept, not_spd = F) when every track is bad.  A status path, not a fault."""
    prob, bad, good, ref = wc.not_spd_case()
    for what in ("update_problem", "load/run/result"):
        if what == "update_problem":
            res = eng.update_problem(prob)
        else:
            eng.load(prob)
            eng.run()
            res = eng.result()
        codes = eng.gate_codes()[0]
        print(f"not SPD, {what}: codes {codes.tolist()} status {res.status} not_spd {res.stats['not_spd']}", flush=True)
        expected = np.full(prob.F, 2, dtype=np.uint8)
        expected[good] = ref["accepted"]
        assert np.array_equal(codes, expected) and (codes[wc.wide(prob)] == 2).sum() == int(bad.sum()) > 0
        assert res.status == ref["status"] == 0
        assert res.stats["not_spd"] == int(bad.sum()) and res.stats["n_rejected"] == int(ref["n_rejected"])
        assert np.array_equal(res.accepted[good], ref["accepted"]) and not res.accepted[bad].any()
        e_dx = rel_err(res.dx, ref["dx"])
        i = 15 + 6 * wc.NOT_SPD_CLONE
        keep = np.r_[0:i, i + 6:prob.d]                    # (the -I block dominates |P|: the error is taken without the cut-off clone too)
        e_P = max(rel_err(res.P_new, ref["P_new"]), rel_err(res.P_new[np.ix_(keep, keep)], ref["P_new"][np.ix_(keep, keep)]))
        print(f"not SPD, {what}: dx {e_dx:.2e} P+ {e_P:.2e}", flush=True)
        assert e_dx < TOL and e_P < TOL
    # every track bad: nothing to update with
    allbad, bad16, _, _ = wc.not_spd_case(16)
    res = eng.update_problem(allbad)
    assert bad16.all() and res.status == _ffi.NOOP
    assert np.array_equal(eng.gate_codes()[0], np.full(allbad.F, 2, dtype=np.uint8))
    assert res.stats["not_spd"] == allbad.F and res.stats["n_accepted"] == 0 and res.stats["n_rejected"] == 0
    assert not res.dx.any() and np.array_equal(res.P_new, allbad.P)


# ---- 10: what is refused ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    good, ref = wc.synth_case("first")
    with _engine(max_clones=66) as e:
        long65 = synth.make_problem(66, 1, 65, seed=27)
        assert _code(e.update_problem, long65) == _ffi.ERR_ARG                       # 65 views
        _one_shot(e, good, ref, "after 65 views")
        assert _code(e.tracks_observe, [1], np.zeros((1, 2)), np.ones(1)) == _ffi.ERR_ARG      # no track store on a wide context
        assert _code(e.tracks_reset) == _ffi.ERR_ARG
        _one_shot(e, good, ref, "after tracks_observe")
        e.load(good)
        assert _code(e.run_compress) == _ffi.ERR_STATE                               # no sharded update with a wide track loaded
        e.run()
        _hold(e.result(), ref, "after run_compress")
    with _engine(max_clones=34, dtype="f32") as e:
        views32 = synth.make_problem(34, 2, 32, seed=28)
        assert _code(e.update_problem, views32) == _ffi.ERR_ARG                      # the f32 stack keeps 31 views
        narrow = synth.make_problem(34, 8, 31, seed=29)
        out = oracle.update(narrow, dense_noise=False)
        res = e.update_problem(narrow)
        assert res.status == out["status"] and np.array_equal(res.accepted, out["accepted"])
        assert rel_err(res.dx, out["dx"]) < 1e-4 and rel_err(res.P_new, out["P_new"]) < 1e-5       # (the f32 mode's tolerances)
    from msckf_amd.api import UpdateEngine
    with pytest.raises(ValueError):
        UpdateEngine(max_clones=66, max_features=8, max_track=65)


# ---- 11: capacity alone changes nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_A", "edge_long_tracks", "edge_mixed_spans", "edge_null_pose"])
def test_capacity_alone_changes_nothing(name):
    """The same batch on a context created for wide tracks and on one created for the narrow kernels' limit (31 views:
    edge_long_tracks holds tracks of 31): dx, P+ and the mask bit for bit."""
    prob, z = load_golden(name)
    with _engine(max_clones=31, max_features=512, max_track=64) as a, _engine(max_clones=31, max_features=512, max_track=31) as b:
        ra, rb = a.update_problem(prob), b.update_problem(prob)
        assert a.debug_split() == b.debug_split()
    assert ra.status == rb.status == int(z["status"])
    assert np.array_equal(ra.dx, rb.dx) and np.array_equal(ra.P_new, rb.P_new) and np.array_equal(ra.accepted, rb.accepted)
    assert np.array_equal(ra.accepted, z["accepted"])
    assert rel_err(ra.dx, z["dx"]) < TOL and rel_err(ra.P_new, z["P_new"]) < TOL
