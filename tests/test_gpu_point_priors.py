"""Priors on the tracks' points (`msckf_set_point_priors`, `msckf_update_prior`, `k_feature_prior`) on the device, against
the restatement of tests/prior_ref.py (not the reference: every track of the reference is a track of an unknown point).
The shapes, their seeds and prior draws: prior_ref.SHAPES, checked on the CPU by tests/test_prior_ref.py.

Tolerances are the project's: dx / P+ 1e-8, gamma rtol 1e-9, the mask equal; the prior distance 1e-9 relative; robust weights
to robust_ref.close.  Every case goes through the one-shot call and through load / set / run, which agree bit for bit."""
import functools

import numpy as np
import pytest

import prior_ref as pr
import robust_ref as rr
from conftest import rel_err
from msckf_amd import _ffi, synth
from oracle import msckf_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 1e-8              # tests/test_gpu_parity.py TOL
GAMMA_RTOL = 1e-9
D2_RTOL = 1e-9
_engines = {}


def _engine(name):
    from msckf_amd.api import UpdateEngine
    if name not in _engines:
        N, F, M, _, plan, _ = pr.SHAPES[name]
        _engines[name] = UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan)
    e = _engines[name]
    e.set_robust(None)
    return e


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@functools.lru_cache(maxsize=None)
def _problem(name):
    return pr.make_shape(name)


@functools.lru_cache(maxsize=None)
def _priors(name, at_mean=False):
    return pr.shape_priors(name, _problem(name), at_mean)


@functools.lru_cache(maxsize=None)
def _ref(name, at_mean=False):
    return pr.update(_problem(name), _priors(name, at_mean))


def _with(prob, pri, **kw):
    return synth.UpdateProblem(**{**prob.__dict__, "point_prior": pri, **kw})


def _same(a, b):
    return a.status == b.status and np.array_equal(a.accepted, b.accepted) and np.array_equal(a.dx, b.dx) and \
        np.array_equal(a.P_new, b.P_new)


def _against(res, gamma, ref):
    assert res.status == ref["status"] == 0
    nz = ref["gamma"] != 0
    print("gamma", float(np.max(np.abs(gamma[nz] - ref["gamma"][nz]) / ref["gamma"][nz])), "dx", rel_err(res.dx, ref["dx"]),
          "P", rel_err(res.P_new, ref["P_new"]))
    assert np.array_equal(res.accepted, ref["accepted"])
    assert np.allclose(gamma, ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
    assert res.n_rejected == ref["n_rejected"]


def _rows(prob, pri, accepted):
    lens = np.diff(prob.view_ptr)
    q = np.where(pri.has.astype(bool), 2 * lens, 2 * lens - 3)
    return int(q[accepted.astype(bool)].sum())


def _resident(e, prob):
    e.load(prob)
    e.run()
    return e.result(), e.debug_gate()[0]


def _check_form(e, name):
    s = e.debug_split()
    print(name, s)
    lens = np.diff(_problem(name).view_ptr)
    has = _priors(name).has.astype(bool)
    if name == "band":
        assert (s["band_plan"], s["sweep_mode"]) == (1, 0) and lens[has].max() == 10, s      # 23 rows in the 24-row form; 20-row blocks
    if name == "tiles90":
        assert (s["band_plan"], s["sweep_mode"]) == (1, 2) and s["long_tracks"] == 0, s      # 90-column tiles
    if name == "split_beside":
        assert s["long_tracks"] > 0, s                        # long plain tracks are split beside short prior tracks
    if name in ("split_beside_long", "thirty"):
        assert s["long_tracks"] == 0, s                       # a long prior track keeps one block, its batch one plan


# ---- 1: every shape, as drawn and linearised at the mean ---------------------------------------------------------------------------
@pytest.mark.parametrize("at_mean", [False, True])
@pytest.mark.parametrize("name", list(pr.SHAPES))
def test_priors_equal_the_restatement(name, at_mean):
    e, prob, pri, ref = _engine(name), _problem(name), _priors(name, at_mean), _ref(name, at_mean)
    res = e.update_problem(_with(prob, pri))
    g, d2 = e.debug_gate()[0], e.prior_distance()
    _check_form(e, name)
    _against(res, g, ref)
    assert res.stats["stacked_rows"] == _rows(prob, pri, ref["accepted"])
    d2_ref = pr.prior_distance(prob, pri)
    if at_mean:
        print("d2 worst", float(d2.max()))
        assert np.all(d2 <= 1e-18)                            # 0 to rounding
    else:
        print("d2 rel", float(np.max(np.abs(d2 - d2_ref)[d2_ref > 0] / d2_ref[d2_ref > 0])))
        assert np.allclose(d2, d2_ref, rtol=D2_RTOL, atol=0.0)
    plain = oracle.update(prob)
    if plain["status"] == 0:
        assert not np.array_equal(plain["accepted"], ref["accepted"]) or rel_err(res.dx, plain["dx"]) > 1e-6   # (the priors did something)
    rres, rg = _resident(e, _with(prob, pri))
    assert _same(rres, res) and np.array_equal(rg, g) and np.array_equal(e.prior_distance(), d2)
    e.run()                                                   # a second run of the batch: the same bits (nothing was overwritten)
    assert _same(e.result(), res) and np.array_equal(e.debug_gate()[0], g)


def test_a_one_view_batch_gives_rows_only_with_priors():
    e, prob = _engine("one_view"), _problem("one_view")
    assert e.update_problem(prob).status == 1                 # 2M - 3 < 0: a no-op (MSCKF.py:584-585)
    res = e.update_problem(_with(prob, _priors("one_view")))
    assert res.status == 0 and res.stats["stacked_rows"] == 2 * int(res.accepted.sum()) > 0


# ---- 2: no priors in force -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.SHAPES))
def test_unchanged_without_priors(name):
    """`has` all 0, a cleared setting and NULL are bitwise the run without priors, one-shot and resident."""
    e, prob, pri = _engine(name), _problem(name), _priors(name)
    F = prob.F
    none = synth.PointPriors(np.zeros(F, dtype=np.uint8), pri.mean, pri.cov)
    base = e.update_problem(prob)
    g0 = e.debug_gate()[0]
    res = e.update_problem(_with(prob, none))
    assert _same(res, base) and np.array_equal(e.debug_gate()[0], g0)
    rbase, rg0 = _resident(e, prob)
    assert _same(rbase, base) or base.status != 0
    rres, rg = _resident(e, _with(prob, none))
    assert _same(rres, rbase) and np.array_equal(rg, rg0)
    e.load(prob)
    e.set_point_priors(pri)
    e.run()
    assert (not _same(e.result(), rbase)) or rbase.status != 0
    e.set_point_priors(None)                                  # cleared
    e.run()
    assert _same(e.result(), rbase) and np.array_equal(e.debug_gate()[0], rg0)
    e.set_point_priors(pri)
    e.set_point_priors(none)                                  # no track named: cleared as well
    e.run()
    assert _same(e.result(), rbase) and np.array_equal(e.debug_gate()[0], rg0)
    assert _code(e.prior_distance) == _ffi.ERR_STATE          # the last run had no priors


# ---- 3: with the per-view options ------------------------------------------------------------------------------------------------
def test_heterogeneous_view_sigma_with_priors():
    name = "band"
    e, prob, pri = _engine(name), _problem(name), _priors(name)
    vs = pr.het_sigma(prob, pr.shape_seed(name) + 1)
    ref = pr.update(prob, pri, vs)
    p = _with(prob, pri, view_sigma=vs)
    res = e.update_problem(p)
    g = e.debug_gate()[0]
    _against(res, g, ref)
    assert not np.array_equal(res.dx, e.update_problem(_with(prob, pri)).dx)      # (the weights did something)
    rres, rg = _resident(e, p)
    assert _same(rres, res) and np.array_equal(rg, g)


@pytest.mark.parametrize("at_mean", [False, True])
def test_huber_with_priors(at_mean):
    """The robust loss weights views, not prior rows; under `at_mean` s_v is formed at the substituted point K1 uses."""
    name = "one_chunk"
    e, prob, pri = _engine(name), _problem(name), _priors(name, at_mean)
    k = 0.02               # (the shape has no outliers: a scale inside its whitened residual norms -- median 0.009, largest 0.059)
    wt = rr.weights(pr.linearised(prob, pri), "huber", k, rr.W_MIN)
    ref = pr.update(prob, pri, view_sigma=float(prob.sigma) / wt["w"])        # (views times w_v; the prior rows as they are)
    assert ref["status"] == 0 and pr.clear_of_threshold(ref) and wt["n_down"] > 0
    if at_mean:
        own = rr.weights(prob, "huber", k, rr.W_MIN)
        assert not rr.close(own["s"], wt["s"])                # (the substitution moves the residual norms)
    e.set_robust("huber", k, rr.W_MIN)
    try:
        res = e.update_problem(_with(prob, pri))
        g, vw = e.debug_gate()[0], e.view_weights()
        print("w worst", rr.worst(vw["w"], wt["w"]), "s worst", rr.worst(vw["s"], wt["s"]))
        assert rr.close(vw["w"], wt["w"]) and rr.close(vw["s"], wt["s"]) and vw["n_down"] == wt["n_down"]
        _against(res, g, ref)
        rres, rg = _resident(e, _with(prob, pri))
        rvw = e.view_weights()
        assert _same(rres, res) and np.array_equal(rg, g) and np.array_equal(rvw["w"], vw["w"]) and np.array_equal(rvw["s"], vw["s"])
    finally:
        e.set_robust(None)


# ---- 4: the caller's order -----------------------------------------------------------------------------------------------------
def test_caller_order_shuffled():
    name = "band"
    e, prob, pri, ref = _engine(name), _problem(name), _priors(name), _ref(name)
    res = e.update_problem(_with(prob, pri))
    g, d2 = e.debug_gate()[0], e.prior_distance()
    perm = np.random.default_rng(5).permutation(prob.F)
    shuffled = _with(prob, pri).take(perm)
    assert np.array_equal(shuffled.point_prior.has, pri.has[perm])
    sres = e.update_problem(shuffled)
    sg = e.debug_gate()[0]
    assert sres.status == 0 and np.array_equal(sres.accepted, res.accepted[perm])
    assert np.array_equal(sg, g[perm]) and np.array_equal(e.prior_distance(), d2[perm])
    assert rel_err(sres.dx, ref["dx"]) < TOL and rel_err(sres.P_new, ref["P_new"]) < TOL


# ---- 5: selection, then run ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at_mean", [False, True])
def test_selection_then_run(at_mean):
    """run_select knows nothing of priors: the valid subset at the refreshed points, the prior rows carrying the offset."""
    name = "band"
    e, prob, pri = _engine(name), _problem(name), _priors(name, at_mean)
    tracks = synth.make_tracks(prob, pr.shape_seed(name), lost_fraction=0.6)
    params = synth.SelectParams(min_parallax_deg=8.0)
    exp = oracle.select_features(prob, tracks, params)
    valid = np.nonzero(exp["flags"] & 1)[0]
    assert 0 < valid.size < prob.F and pri.has[valid].any()
    chained = prob.take(valid)
    chained.idp_m, chained.idp_rho = exp["idp_m"][valid], exp["idp_rho"][valid]
    cpri = pri.take(valid)
    ref = pr.update(chained, cpri)
    assert ref["status"] == 0 and pr.clear_of_threshold(ref)
    e.load(prob)
    e.set_tracks(tracks)
    e.set_point_priors(pri)                                   # (before or after set_tracks / run_select)
    e.run_select(params, prob.K)
    e.run()
    res = e.result()
    assert np.array_equal(e.selection().flags & 1, exp["flags"] & 1)
    assert res.status == 0 and np.array_equal(res.accepted[valid], ref["accepted"]) and res.n_rejected == ref["n_rejected"]
    assert not res.accepted[np.setdiff1d(np.arange(prob.F), valid)].any()     # a skipped track stays skipped
    assert np.allclose(e.debug_gate()[0][valid], ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
    d2, d2_ref = e.prior_distance(), pr.prior_distance(chained, cpri)
    assert not d2[np.setdiff1d(np.arange(prob.F), valid)].any()
    if at_mean:
        assert np.all(d2 <= 1e-18)
    else:
        assert np.allclose(d2[valid], d2_ref, rtol=D2_RTOL, atol=0.0)
    e.replan()                                                # the plan over the valid tracks only: the same update
    e.run()
    again = e.result()
    assert np.array_equal(again.accepted, res.accepted)
    assert rel_err(again.dx, ref["dx"]) < TOL and rel_err(again.P_new, ref["P_new"]) < TOL


# ---- 6: the track store -------------------------------------------------------------------------------------------------------------
def test_store_batch_with_priors():
    """A batch of the track store with priors equals, bit for bit, the same batch through set_features + set_point_priors on a
    second engine -- a track created in the newest clone only among them, linearised at its landmark's mean."""
    from msckf_amd.api import UpdateEngine
    from test_gpu_tracks import _grow, _small, _store_batch
    p, uv = _small(6, 10, seed=11)
    ids = [3, 14, 15, 9, 26, 5, 35, 8, 97, 12]
    views = [[0, 1, 2, 3, 4, 5], [0, 2, 3, 5], [1, 2, 3], [2, 3, 4, 5], [0, 1, 2, 3, 4], [3, 4, 5], [0, 1, 4, 5], [1, 2, 3, 4, 5],
             [5], [2, 3, 4]]                                  # 97: seen in the newest clone only
    params = synth.SelectParams(min_frames_lost=1, min_frames_tracked=2, use_parallax=True, min_parallax_deg=0.0)
    kw = dict(max_clones=8, max_features=16, max_track=8)
    Kinv = np.linalg.inv(p.K)
    with UpdateEngine(**kw) as eng, UpdateEngine(**kw) as eng_b:
        _grow(eng, p, uv, views, ids)
        P = eng.covariance()
        order = eng.load_tracks_where()
        assert sorted(order.tolist()) == sorted(ids)
        eng.run_select(params, p.K)                           # the refresh persists in the store (MSCKF.py:488)
        sel = eng.selection()
        assert np.array_equal(eng.load_tracks_where(), order)  # the batch again: no selection in force
        tr, b = _store_batch(eng, order)
        F = len(order)
        refreshed = (sel.flags & _ffi.SEL_REFRESHED) != 0
        one = int(np.nonzero(order == 97)[0][0])
        assert not refreshed[one] and len(tr[one]["slots"]) == 1
        has = ~refreshed | (np.arange(F) % 2 == 0)            # every track without a triangulated point is a landmark
        rng = np.random.default_rng(17)
        mean, cov = np.zeros((F, 3)), np.zeros((F, 3, 3))
        for j in range(F):
            L = 0.05 * (np.eye(3) + 0.3 * np.tril(rng.standard_normal((3, 3)), -1))
            cov[j] = L @ L.T
            cov[j] = (cov[j] + cov[j].T) / 2
            if refreshed[j]:
                mean[j] = b["idp_base"][j] + b["idp_m"][j] / b["idp_rho"][j] + L @ rng.standard_normal(3)
            else:                                             # along the first view's ray, 8 m out
                s = int(tr[j]["slots"][0])
                ray = p.cam_R[s] @ (Kinv @ np.append(tr[j]["uv"].reshape(-1, 2)[0], 1.0))
                mean[j] = p.cam_t[s] + 8.0 * ray / np.linalg.norm(ray)
        pri = synth.PointPriors(has, mean, cov, at_mean=True)
        eng.set_point_priors(pri)
        eng.run()
        res, g, d2 = eng.result(), eng.debug_gate()[0], eng.prior_distance()
        assert res.status == 0 and res.accepted[one] == 1 and np.all(np.isfinite(g[has]))
        # the same batch through the host's door
        eng_b.set_prior(P, p.gravity, p.K, p.sigma, p.cam_R, p.cam_t)
        prob = synth.UpdateProblem(P=P, cam_R=p.cam_R, cam_t=p.cam_t, cam_R0=p.cam_R, cam_t0=p.cam_t, gravity=p.gravity, K=p.K,
                                   sigma=p.sigma, view_ptr=b["view_ptr"], obs_uv=b["obs_uv"], obs_slot=b["obs_slot"],
                                   idp_base=b["idp_base"], idp_m=b["idp_m"].copy(), idp_rho=b["idp_rho"].copy())
        eng_b.set_features(prob)
        eng_b.set_point_priors(pri)
        eng_b.run()
        res_b = eng_b.result()
        assert _same(res, res_b) and np.array_equal(g, eng_b.debug_gate()[0], equal_nan=True)
        assert np.array_equal(d2, eng_b.prior_distance())
        # the store's rows were only read
        tr2, _ = _store_batch(eng, order)
        assert all(np.array_equal(x["idp_m"], y["idp_m"]) and np.array_equal(x["idp_rho"], y["idp_rho"]) for x, y in zip(tr, tr2))


# ---- 7: a prior too loose to see -----------------------------------------------------------------------------------------------
def test_rank_deficient_prior_is_rejected():
    name = "one_view"
    e, prob = _engine(name), _problem(name)
    pri = pr.shape_priors(name, prob)
    j = int(np.nonzero(_ref(name)["accepted"])[0][0])         # a track the gate accepts with its drawn prior
    pri.cov[j] = 1e40 * np.eye(3)
    rest = np.array([k for k in range(prob.F) if k != j])
    ref = pr.update(prob.take(rest), pri.take(rest))
    res = e.update_problem(_with(prob, pri))
    assert res.status == 0 and res.accepted[j] == 0 and np.array_equal(res.accepted[rest], ref["accepted"])
    assert res.n_rejected == ref["n_rejected"] + 1 and res.stats["stacked_rows"] == 2 * int(ref["accepted"].sum())
    assert np.allclose(e.debug_gate()[0][rest], ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
    rres, _ = _resident(e, _with(prob, pri))
    assert _same(rres, res)


# ---- 8: lifetime and errors --------------------------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    with pytest.raises(_ffi.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _raw_set(e, pri, flags=None, reserved=0):
    import ctypes as C
    pc, keep = e._point_priors(pri, pri.F)
    if flags is not None:
        pc.flags = flags
    pc.reserved = reserved
    rc = e._lib.msckf_set_point_priors(e._h, C.byref(pc))
    del keep
    return rc


def test_lifetime_and_errors():
    from msckf_amd.api import UpdateEngine
    name = "band"
    prob, pri, ref = _problem(name), _priors(name), _ref(name)
    N, F, M, _, plan, _ = pr.SHAPES[name]
    with UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan) as e:
        assert _code(e.set_point_priors, pri) == _ffi.ERR_STATE      # before any batch
        e.set_state(prob)
        assert _code(e.set_point_priors, pri) == _ffi.ERR_STATE      # a state, no batch
        plain, pg = _resident(e, prob)
        assert _code(e.prior_distance) == _ffi.ERR_STATE
        e.set_point_priors(pri)
        assert _code(e.prior_distance) == _ffi.ERR_STATE             # set, not run
        e.run()
        with_p, wg = e.result(), e.debug_gate()[0]
        _against(with_p, wg, ref)
        d2 = e.prior_distance()

        def unchanged():
            e.run()
            return _same(e.result(), with_p) and np.array_equal(e.debug_gate()[0], wg) and np.array_equal(e.prior_distance(), d2)
        # every refusal, with the priors in force as they were
        j = int(np.nonzero(pri.has)[0][3])
        for what in ("nan_mean", "nan_cov", "asymmetric", "indefinite", "zero"):
            bad = synth.PointPriors(pri.has, pri.mean.copy(), pri.cov.copy())
            if what == "nan_mean":
                bad.mean[j, 1] = np.nan
            elif what == "nan_cov":
                bad.cov[j, 2, 2] = np.inf
            elif what == "asymmetric":
                bad.cov[j, 0, 1] = np.nextafter(bad.cov[j, 0, 1], 1.0)
            elif what == "indefinite":
                bad.cov[j] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
            else:
                bad.cov[j] = 0.0
            assert _code(e.set_point_priors, bad) == _ffi.ERR_ARG, what
            assert unchanged(), what
        assert _raw_set(e, pri, reserved=1) == _ffi.ERR_ARG and _raw_set(e, pri, flags=2) == _ffi.ERR_ARG and unchanged()
        with pytest.raises(ValueError):
            e.set_point_priors(pri.subset(0, F - 1))
        # sharded calls answer ERR_STATE while priors are in force, and work again once they are cleared
        assert _code(e.run_compress) == _ffi.ERR_STATE
        assert unchanged()
        # run_timed goes through the same K1
        e.run_timed(2)
        assert _same(e.result(), with_p)
        # NULL clears
        e.set_point_priors(None)
        e.run()
        assert _same(e.result(), plain) and np.array_equal(e.debug_gate()[0], pg)
        e.run_compress()
        # ... so does a new batch
        e.set_point_priors(pri)
        e.set_features(prob)
        e.run()
        assert _same(e.result(), plain)
        # ... and a new state
        e.set_point_priors(pri)
        e.set_state(prob)
        e.run()
        assert _same(e.result(), plain)
        assert _code(e.prior_distance) == _ffi.ERR_STATE
        # poses and rows updates leave them with the batch
        e.set_point_priors(pri)
        e.set_poses(prob.cam_R, prob.cam_t, prob.cam_R0, prob.cam_t0)
        assert unchanged()
        # under a group exchange: refused
        e.set_point_priors(None)
        e.set_group_exchange(True)
        e.load(prob)
        assert _code(e.set_point_priors, pri) == _ffi.ERR_STATE
        e.set_group_exchange(False)
    # a prior on a track of more than 30 views, and an f32 context
    with UpdateEngine(max_clones=31, max_features=4, max_track=31, plan="band") as e:
        p31 = synth.make_problem(31, 4, 31, seed=3)
        e.load(p31)
        long_pri = pr.draw_priors(p31, 1, "all")
        assert _code(e.set_point_priors, long_pri) == _ffi.ERR_ARG
        e.run()
        assert e.result().status == 0
    with UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan, dtype="f32") as e:
        e.load(prob)
        assert _code(e.set_point_priors, pri) == _ffi.ERR_ARG
        assert _code(e.update_problem, _with(prob, pri)) == _ffi.ERR_ARG


# ---- 9: the reference-shaped adapter ---------------------------------------------------------------------------------------------
def test_reference_shaped_adapter_takes_a_mapping():
    """`update(filt, features, point_priors={key: (mean, cov)})`: features the mapping does not name are plain tracks; the
    covariance the filter is left with is the restatement's."""
    from conftest import load_golden
    from msckf_amd.api import UpdateEngine
    from test_host_logic import make_reference_shaped
    prob, gold = load_golden("edge_some_rejected")
    filt, feats = make_reference_shaped(prob, gold)
    keys = list(feats)
    drawn = pr.draw_priors(prob, 23, "half")
    mapping = {k: (drawn.mean[j], drawn.cov[j]) for j, k in enumerate(keys) if drawn.has[j]}
    ref = pr.update(prob, drawn)
    assert ref["status"] == 0 and pr.clear_of_threshold(ref) and 0 < ref["n_rejected"] < prob.F
    M = int(np.diff(prob.view_ptr).max())
    with UpdateEngine(max_clones=prob.N, max_features=prob.F, max_track=max(M, 2)) as e:
        assert e.update(filt, feats, point_priors=mapping) == 0
        assert np.allclose(e.debug_gate()[0], ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert filt.number_of_residuals_discarded_for_gasting_test == ref["n_rejected"]
    assert rel_err(filt.state.covariance, ref["P_new"]) < TOL
