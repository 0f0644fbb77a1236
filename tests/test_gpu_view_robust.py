"""Robust per-view weights in front of K1 (`msckf_set_robust`, `k_robust`) on the device: every `k_feature` form, the wide
kernel and every K5 plan, both upload paths, repeated runs, the selection with refinement, both dtypes, the shards and the
track store -- against the restatement of tests/robust_ref.py (not the reference: it has no robust loss).  The shapes, their
seeds and what makes them cases: robust_ref.SHAPES, checked on the CPU by tests/test_robust_ref.py.

Tolerances: w and s against the helper |diff| <= 1e-12 (1 + |ref|) (robust_ref.close: its derivation); dx / P+ 1e-8, gamma
rtol 1e-9, the mask equal (the project's TOL / GAMMA_RTOL); the f32 mode at its 1e-4 / 1e-5.  Every figure is printed
before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import robust_ref as rr
import weighted_ref as wr
from conftest import rel_err
from msckf_amd import _ffi, synth

pytestmark = pytest.mark.gpu

TOL = 1e-8              # tests/test_gpu_parity.py TOL
GAMMA_RTOL = 1e-9
TOL32_DX, TOL32_P = 1e-4, 1e-5      # the f32 mode's flat tolerance

# what msckf_debug_split says of the shape: (band_plan, sweep_mode, long tracks split), as tests/test_gpu_view_sigma.py has it;
# wide: one block per track on the merge tree (tests/test_gpu_wide_tracks.py)
FORMS = {
    "one_chunk": (1, 0, False),
    "band": (1, 0, False),
    "tiles90": (1, 2, False),
    "ring": (1, 1, False),
    "split": (1, 0, True),
    "unsplit31": (0, -1, False),
    "wide": (0, None, False),
}
LONGEST_M = {"one_chunk": (1, 10), "band": (1, 10), "tiles90": (11, 15), "ring": (1, 10), "split": (16, 31), "unsplit31": (31, 31),
             "wide": (32, 64)}
_engines = {}


def _engine(name, dtype="f64"):
    from msckf_amd.api import UpdateEngine
    key = (name, dtype)
    if key not in _engines:
        N, F, M, _, plan = rr.SHAPES[name]
        _engines[key] = UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan, dtype=dtype)
    e = _engines[key]
    e.set_robust(None)
    return e


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def _with(prob, view_sigma, **kw):
    return synth.UpdateProblem(**{**prob.__dict__, "view_sigma": view_sigma, **kw})


def _check_form(e, name):
    s = e.debug_split()
    band_plan, sweep_mode, split = FORMS[name]
    print(name, s)
    assert s["band_plan"] == band_plan and (sweep_mode is None or s["sweep_mode"] == sweep_mode), s
    assert (s["long_tracks"] > 0) == split, s
    M = int(np.diff(rr.make_shape(name).view_ptr).max())
    lo, hi = LONGEST_M[name]
    assert lo <= M <= hi, M


def _same(a, b):
    return a.status == b.status and np.array_equal(a.accepted, b.accepted) and np.array_equal(a.dx, b.dx) and \
        np.array_equal(a.P_new, b.P_new)


def _against(res, gamma, ref, tol_dx=TOL, tol_P=TOL):
    assert res.status == ref["status"] == 0
    print("gamma", float(np.max(np.abs(gamma - ref["gamma"]) / ref["gamma"])), "dx", rel_err(res.dx, ref["dx"]),
          "P", rel_err(res.P_new, ref["P_new"]))
    assert np.array_equal(res.accepted, ref["accepted"])
    assert np.allclose(gamma, ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert rel_err(res.dx, ref["dx"]) < tol_dx and rel_err(res.P_new, ref["P_new"]) < tol_P


def _weights_against(vw, wt, what=""):
    print(what, "w worst", rr.worst(vw["w"], wt["w"]), "s worst", rr.worst(vw["s"], wt["s"]), "n_down", vw["n_down"], wt["n_down"])
    assert vw["w"].shape == wt["w"].shape and vw["s"].shape == wt["s"].shape
    assert rr.close(vw["w"], wt["w"]) and rr.close(vw["s"], wt["s"])
    assert vw["n_down"] == wt["n_down"]


def _resident(e, prob):
    e.load(prob)
    e.run()
    return e.result(), e.debug_gate()[0], e.view_weights()


def _same_weights(a, b):
    return np.array_equal(a["w"], b["w"]) and np.array_equal(a["s"], b["s"]) and a["n_down"] == b["n_down"]


def _case(name, which, dtype="f64", tol_dx=TOL, tol_P=TOL):
    """One-shot and resident under the variant's loss against the helper; returns the one-shot result."""
    loss, k, vs = rr.variant(name, which)
    e, prob = _engine(name, dtype), rr.make_shape(name)
    ref, wt = rr.robust_ref(name, which)
    p = _with(prob, vs)
    e.set_robust(loss, k, rr.W_MIN)
    res = e.update_problem(p)
    g, vw = e.debug_gate()[0], e.view_weights()
    _check_form(e, name)
    _weights_against(vw, wt, f"{name} {which} one-shot")
    _against(res, g, ref, tol_dx, tol_P)
    resc = rr.rescued(name, which)
    assert resc.size >= 1 and np.all(res.accepted[resc] == 1)
    rres, rg, rvw = _resident(e, p)
    assert _same(rres, res) and np.array_equal(rg, g) and _same_weights(rvw, vw)
    e.set_robust(None)
    return res


# ---- 1: per shape, Huber ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rr.SHAPES))
def test_huber_on_every_shape(name):
    res = _case(name, "huber")
    e = _engine(name)
    plain = e.update_problem(rr.make_shape(name))
    assert int(plain.accepted.sum()) < int(res.accepted.sum())              # (the option did something)


# ---- 2: the other loss, the other base ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_chunk", "split"])
def test_cauchy(name):
    _case(name, "cauchy")


@pytest.mark.parametrize("name", ["band", "wide"])
def test_huber_on_the_heterogeneous_base(name):
    _case(name, "huber_het")


# ---- 3: nothing to down-weight, and off again ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band", "split"])
def test_a_k_beyond_every_residual_is_bitwise_the_run_without_the_option(name):
    e, prob = _engine(name), rr.make_shape(name)
    s = rr.weights(prob, "huber", rr.HUBER_K, rr.W_MIN)["s"]
    base = e.update_problem(prob)
    g0 = e.debug_gate()[0]
    e.load(prob)
    e.run()
    rbase, rg0 = e.result(), e.debug_gate()[0]
    e.set_robust("huber", 2.0 * float(s.max()), rr.W_MIN)
    res = e.update_problem(prob)
    vw = e.view_weights()
    assert _same(res, base) and np.array_equal(e.debug_gate()[0], g0)
    assert np.array_equal(vw["w"], np.ones(s.size)) and vw["n_down"] == 0 and rr.close(vw["s"], s)
    rres, rg, rvw = _resident(e, prob)
    assert _same(rres, rbase) and np.array_equal(rg, rg0) and _same_weights(rvw, vw)
    # a loss that bites, then off: the earlier run without the option, bit for bit
    e.set_robust("huber", rr.HUBER_K, rr.W_MIN)
    e.run()
    assert not _same(e.result(), rbase)
    e.set_robust(None)
    e.run()
    assert _same(e.result(), rbase) and np.array_equal(e.debug_gate()[0], rg0)
    assert _same(e.update_problem(prob), base)


# ---- 4: repeated runs recompute, never compound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band", "split"])
def test_repeated_runs_form_the_same_weights(name):
    e = _engine(name)
    prob = _with(rr.make_shape(name), rr.het_sigma(name))
    e.set_robust("huber", rr.HUBER_K, rr.W_MIN)
    first, g, vw = _resident(e, prob)
    assert vw["n_down"] > 0
    e.run()
    e.run()
    e.run_timed(3)
    e.run()
    assert _same(e.result(), first) and np.array_equal(e.debug_gate()[0], g) and _same_weights(e.view_weights(), vw)
    e.run_timed(2, stages=True)
    assert _same(e.result(), first) and _same_weights(e.view_weights(), vw)
    e.set_robust(None)


# ---- 5: behind the selection and its refinement -----------------------------------------------------------------------------------------
def test_weights_at_the_selections_refreshed_points():
    name = "band"
    e, prob = _engine(name), rr.make_shape(name)
    vs = rr.het_sigma(name)
    tracks = synth.make_tracks(prob, rr.shape_seed(name), lost_fraction=0.6)
    params = synth.SelectParams(min_parallax_deg=8.0, refine_iters=8)
    e.set_robust("huber", rr.HUBER_K, rr.W_MIN)
    e.load(_with(prob, vs))
    e.set_tracks(tracks)
    e.run_select(params, prob.K)
    e.run()
    res, sel, vw = e.result(), e.selection(), e.view_weights()
    valid = (sel.flags & _ffi.SEL_VALID) != 0
    fresh = (sel.flags & _ffi.SEL_REFRESHED) != 0
    # (a valid track whose triangulated point fails the image test keeps its point: MSCKF.py:483-488)
    assert 0 < int(valid.sum()) < prob.F and np.any(fresh & valid) and np.any(sel.flags & _ffi.SEL_REFINED)
    at = _with(prob, vs)
    at.idp_m = np.where(fresh[:, None], sel.idp_m, prob.idp_m)
    at.idp_rho = np.where(fresh, sel.idp_rho, prob.idp_rho)
    wt = rr.weights(at, "huber", rr.HUBER_K, rr.W_MIN, vs)
    vvalid = np.repeat(valid, np.diff(prob.view_ptr))
    exp = dict(w=np.where(vvalid, wt["w"], wt["b"]), s=np.where(vvalid, wt["s"], 0.0),
               n_down=int(np.count_nonzero(vvalid & (wt["phi"] < 1.0))))
    _weights_against(vw, exp, "selection")
    assert np.array_equal(vw["w"][~vvalid], wt["b"][~vvalid]) and np.all(vw["s"][~vvalid] == 0.0)
    assert exp["n_down"] > 0 and np.all(res.accepted[~valid] == 0)
    e.set_robust(None)


# ---- 6: lifetime and errors ---------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    with pytest.raises(_ffi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def test_lifetime_and_errors():
    from msckf_amd.api import UpdateEngine
    name = "band"
    prob, vs = rr.make_shape(name), rr.het_sigma(name)
    N, F, M, _, plan = rr.SHAPES[name]
    ref, wt = rr.robust_ref(name, "huber")
    ref_het, wt_het = rr.robust_ref(name, "huber_het")
    with UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan) as e:
        assert _code(e.view_weights) == _ffi.ERR_STATE            # nothing loaded
        e.load(prob)
        e.run()
        plain = e.result()
        assert _code(e.view_weights) == _ffi.ERR_STATE            # a run, the option off (as after msckf_create)
        e.set_robust("huber", rr.HUBER_K, rr.W_MIN)
        assert _code(e.view_weights) == _ffi.ERR_STATE            # the option on, no run with it yet
        e.run()
        hub, g, vw = e.result(), e.debug_gate()[0], e.view_weights()
        _weights_against(vw, wt, "lifetime")
        _against(hub, g, ref)
        # each bad parameter: MSCKF_ERR_ARG, and the setting stays
        for kw in (dict(loss=3), dict(loss=-1), dict(loss="huber", k=0.0), dict(loss="huber", k=-1.0), dict(loss="huber", k=np.inf),
                   dict(loss="huber", k=np.nan), dict(loss="cauchy", w_min=0.0), dict(loss="cauchy", w_min=-0.1),
                   dict(loss="cauchy", w_min=1.0000001), dict(loss="cauchy", w_min=np.nan)):
            assert _code(e.set_robust, **kw) == _ffi.ERR_ARG, kw
        rp = _ffi.RobustParamsC(_ffi.ROBUST_CAUCHY, 1, rr.CAUCHY_K, rr.W_MIN)       # reserved != 0
        assert e._lib.msckf_set_robust(e._h, C.byref(rp)) == _ffi.ERR_ARG
        with pytest.raises(ValueError):
            e.set_robust("tukey")
        e.run()
        assert _same(e.result(), hub) and _same_weights(e.view_weights(), vw)
        # a voided run: no weights to read (the rules of result())
        e.set_state(prob)
        assert _code(e.view_weights) == _ffi.ERR_STATE
        # ... but the setting survives set_state and a new batch
        e.run()
        assert _same(e.result(), hub) and _same_weights(e.view_weights(), vw)
        e.set_features(prob)
        assert _code(e.view_weights) == _ffi.ERR_STATE
        e.run()
        assert _same(e.result(), hub) and _same_weights(e.view_weights(), vw)
        # set_view_sigma after it changes the base of the next run; the base itself is not touched by the runs
        e.set_view_sigma(vs)
        e.run()
        het, hg, hvw = e.result(), e.debug_gate()[0], e.view_weights()
        _weights_against(hvw, wt_het, "lifetime, heterogeneous base")
        _against(het, hg, ref_het)
        e.run()
        assert _same(e.result(), het) and _same_weights(e.view_weights(), hvw)
        e.set_view_sigma(None)
        e.run()
        assert _same(e.result(), hub) and _same_weights(e.view_weights(), vw)
        # run_compress goes through the same K1
        e.run_compress()
        assert _same_weights(e.view_weights(), vw)
        # any pointer of the C call may be NULL; then off: the plain run, and no weights to read
        e.run()
        nd = np.zeros(1, dtype=np.int32)
        assert e._lib.msckf_get_view_weights(e._h, None, None, _ffi.iptr(nd)) == 0 and int(nd[0]) == vw["n_down"]
        assert e._lib.msckf_get_view_weights(e._h, None, None, None) == 0
        e.set_robust(None)
        e.run()
        assert _same(e.result(), plain) and _code(e.view_weights) == _ffi.ERR_STATE


# ---- 7: the f32 mode (the weights are fp64 there too) ----------------------------------------------------------------------------------------
def test_huber_on_an_f32_stack():
    _case("band", "huber", "f32", TOL32_DX, TOL32_P)


# ---- 8: two logical shards -------------------------------------------------------------------------------------------------------------------
def test_two_logical_shards_form_their_own_weights():
    """The band shape as 2 shards on one GPU, the loss set once on the context: each shard's K1 reads the weights of its own
    views, the records and the merge know nothing of them."""
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import partition_features
    name = "band"
    prob = rr.make_shape(name)
    ref, wt = rr.robust_ref(name, "huber_het")
    het = _with(prob, rr.het_sigma(name))
    N, F, M, _, plan = rr.SHAPES[name]
    with UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan) as e:
        assert e.band_ok(prob)
        e.set_group_exchange(True)
        e.set_robust("huber", rr.HUBER_K, rr.W_MIN)
        recs, total, acc = [], 0, np.zeros(prob.F, dtype=np.uint8)
        w, s, n_down = np.zeros(wt["w"].size), np.zeros(wt["w"].size), 0
        shards = partition_features(prob.view_ptr, 2)
        assert all(hi > lo for lo, hi in shards)
        for lo, hi in shards:
            e.load(het.subset(lo, hi))
            e.run_compress()
            rec, n = e.export_groups()
            acc[lo:hi] = e.result().accepted
            vw = e.view_weights()
            a, b = int(prob.view_ptr[lo]), int(prob.view_ptr[hi])
            w[a:b], s[a:b] = vw["w"], vw["s"]
            n_down += vw["n_down"]
            recs.append(rec); total += n
        _weights_against(dict(w=w, s=s, n_down=n_down), wt, "shards")
        e.set_state(prob)
        e.merge_groups(np.stack(recs), total)
        res = e.result()
        print("dx", rel_err(res.dx, ref["dx"]), "P", rel_err(res.P_new, ref["P_new"]))
        assert res.status == 0 and np.array_equal(acc, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL


# ---- 9: a batch of the track store -------------------------------------------------------------------------------------------------------------
def test_store_batch_forms_weights_in_its_view_order():
    """A batch of the track store (tracks_observe ... load_tracks_where) under a loss equals, bit for bit, the same batch
    through set_features on a second engine, and its weights are the helper's at the selection's refreshed points."""
    from msckf_amd.api import UpdateEngine
    from test_gpu_tracks import _grow, _small, _store_batch
    p, uv = _small(6, 10, seed=11)
    uv = uv.copy()
    uv[1, 3] += 400.0 * np.array([1.0, -0.7])                  # one gross outlier view
    ids = [3, 14, 15, 9, 26, 5, 35, 8, 97, 12]
    views = [[0, 1, 2, 3, 4, 5], [0, 2, 3, 5], [1, 2, 3], [2, 3, 4, 5], [0, 1, 2, 3, 4], [3, 4, 5], [0, 1, 4, 5], [1, 2, 3, 4, 5],
             [0, 5], [2, 3, 4]]
    params = synth.SelectParams(min_frames_lost=1, min_frames_tracked=2, use_parallax=True, min_parallax_deg=0.0)
    kw = dict(max_clones=8, max_features=16, max_track=8)
    with UpdateEngine(**kw) as eng, UpdateEngine(**kw) as eng_b:
        _grow(eng, p, uv, views, ids)
        P = eng.covariance()
        order = eng.load_tracks_where()
        n = sum(map(len, views))

        def finish(e):
            e.run_select(params, p.K)
            sel = e.selection()
            e.run()
            return sel, e.result(), e.debug_gate()[0]
        plain = finish(eng)
        _, b = _store_batch(eng, order)                         # (the rows as the selection's refresh left them)
        assert int(b["view_ptr"][-1]) == n
        assert np.array_equal(eng.load_tracks_where(), order)
        eng.set_robust("cauchy", rr.CAUCHY_K, rr.W_MIN)
        sel, res, g = finish(eng)
        vw = eng.view_weights()                                 # (the engine counts the views of a store batch)
        assert vw["w"].size == n and vw["s"].size == n
        assert sel.valid.any() and res.status == 0 and not np.array_equal(res.dx, plain[1].dx)
        # the same batch through the host's door
        eng_b.set_prior(P, p.gravity, p.K, p.sigma, p.cam_R, p.cam_t)
        prob = synth.UpdateProblem(P=P, cam_R=p.cam_R, cam_t=p.cam_t, cam_R0=p.cam_R, cam_t0=p.cam_t, gravity=p.gravity, K=p.K,
                                   sigma=p.sigma, view_ptr=b["view_ptr"], obs_uv=b["obs_uv"], obs_slot=b["obs_slot"],
                                   idp_base=b["idp_base"], idp_m=b["idp_m"].copy(), idp_rho=b["idp_rho"].copy())
        eng_b.set_robust("cauchy", rr.CAUCHY_K, rr.W_MIN)
        eng_b.set_features(prob)
        lost, tracked = eng.tracks_counters(order)
        eng_b.set_tracks(synth.TrackTable(line_base=b["line_base"], line_dir=b["line_dir"], line_conf=b["line_conf"],
                                          lost_for=lost, tracked_for=tracked))
        sel_b, res_b, g_b = finish(eng_b)
        assert np.array_equal(sel.flags, sel_b.flags) and np.array_equal(sel.idp_m, sel_b.idp_m)
        assert _same(res, res_b) and np.array_equal(g, g_b) and _same_weights(vw, eng_b.view_weights())
        # ... and against the helper, at the points the selection left
        fresh = (sel.flags & _ffi.SEL_REFRESHED) != 0
        prob.idp_m = np.where(fresh[:, None], sel.idp_m, prob.idp_m)
        prob.idp_rho = np.where(fresh, sel.idp_rho, prob.idp_rho)
        wt = rr.weights(prob, "cauchy", rr.CAUCHY_K, rr.W_MIN)
        vvalid = np.repeat(sel.valid, np.diff(prob.view_ptr))
        exp = dict(w=np.where(vvalid, wt["w"], 1.0), s=np.where(vvalid, wt["s"], 0.0),
                   n_down=int(np.count_nonzero(vvalid & (wt["phi"] < 1.0))))
        _weights_against(vw, exp, "store")
        assert exp["n_down"] > 0
