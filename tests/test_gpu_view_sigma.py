"""Per-view measurement noise (`msckf_set_view_sigma`, `msckf_update_sigma`) on the device: every `k_feature` form and K5
plan, both upload paths, the on-device permutation, the selection, the shards, the track store, both dtypes -- against the
oracle where uniform weights make it the reference, else against its restatement with weights (tests/weighted_ref.py).
The shapes and their seeds: weighted_ref.SHAPES, checked on the CPU by tests/test_weighted_ref.py."""
import functools

import numpy as np
import pytest

import weighted_ref as wr
from conftest import rel_err
from msckf_amd import _ffi, synth
from oracle import msckf_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 1e-8              # tests/test_gpu_parity.py TOL
GAMMA_RTOL = 1e-9
TOL32_DX, TOL32_P = 1e-4, 1e-5      # the f32 mode's flat tolerance

# what msckf_debug_split says of the shape: (band_plan, sweep_mode, long tracks split); the k_feature form follows from the
# longest track (<= 10 views: one chunk; 11 - 15: two chunks; more: the chunked form, split or not)
FORMS = {
    "one_chunk": (1, 0, False),
    "band": (1, 0, False),
    "tiles90": (1, 2, False),
    "ring": (1, 1, False),
    "split": (1, 0, True),
    "unsplit31": (0, -1, False),
}
_engines = {}


def _engine(name, dtype="f64"):
    from msckf_amd.api import UpdateEngine
    key = (name, dtype)
    if key not in _engines:
        N, F, M, _, plan = wr.SHAPES[name]
        _engines[key] = UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan, dtype=dtype)
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@functools.lru_cache(maxsize=None)
def _problem(name):
    return wr.make_shape(name)


def _with(prob, view_sigma, **kw):
    return synth.UpdateProblem(**{**prob.__dict__, "view_sigma": view_sigma, **kw})


@functools.lru_cache(maxsize=None)
def _het(name):
    prob = _problem(name)
    vs = wr.het_sigma(prob, wr.shape_seed(name))
    vs.setflags(write=False)
    return vs


@functools.lru_cache(maxsize=None)
def _het_ref(name):
    return wr.update(_problem(name), _het(name))


def _n_views(prob):
    return int(prob.view_ptr[-1])


def _check_form(e, name):
    s = e.debug_split()
    band_plan, sweep_mode, split = FORMS[name]
    print(name, s)
    assert (s["band_plan"], s["sweep_mode"]) == (band_plan, sweep_mode), s
    assert (s["long_tracks"] > 0) == split, s
    M = int(np.diff(_problem(name).view_ptr).max())
    lo, hi = {"one_chunk": (1, 10), "band": (1, 10), "tiles90": (11, 15), "ring": (1, 10), "split": (16, 31), "unsplit31": (31, 31)}[name]
    assert lo <= M <= hi, M


def _same(a, b):
    return a.status == b.status and np.array_equal(a.accepted, b.accepted) and np.array_equal(a.dx, b.dx) and \
        np.array_equal(a.P_new, b.P_new)


def _against(res, gamma, ref, tol_dx=TOL, tol_P=TOL):
    assert res.status == ref["status"] == 0
    assert np.array_equal(res.accepted, ref["accepted"])
    print("gamma", float(np.max(np.abs(gamma - ref["gamma"]) / ref["gamma"])), "dx", rel_err(res.dx, ref["dx"]),
          "P", rel_err(res.P_new, ref["P_new"]))
    assert np.allclose(gamma, ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert rel_err(res.dx, ref["dx"]) < tol_dx and rel_err(res.P_new, ref["P_new"]) < tol_P


def _resident(e, prob):
    e.load(prob)
    e.run()
    return e.result(), e.debug_gate()[0]


@pytest.mark.parametrize("name", list(wr.SHAPES))
def test_all_ones_are_bitwise_the_unweighted_run(name):
    """sigma_v == sigma for every view: w_v is exactly 1, and dx, P+, the mask and gamma are those of the same engine's run
    without weights -- through the one-shot call and through load / run."""
    e, prob = _engine(name), _problem(name)
    ones = _with(prob, np.full(_n_views(prob), prob.sigma))
    base = e.update_problem(prob)
    g0 = e.debug_gate()[0]
    _check_form(e, name)
    assert base.status == 0
    res = e.update_problem(ones)
    assert _same(res, base) and np.array_equal(e.debug_gate()[0], g0)
    rbase, rg0 = _resident(e, prob)
    rres, rg = _resident(e, ones)
    assert _same(rres, rbase) and np.array_equal(rg, rg0)


@pytest.mark.parametrize("name", list(wr.SHAPES))
def test_uniform_half_sigma_equals_the_oracle_at_half_sigma(name):
    """sigma_v == sigma / 2 for every view is the unweighted update at the global sigma / 2: the oracle as it stands."""
    e, prob = _engine(name), _problem(name)
    ref = oracle.update(_with(prob, None, sigma=prob.sigma / 2), dense_noise=False)
    half = _with(prob, np.full(_n_views(prob), prob.sigma / 2))
    res = e.update_problem(half)
    _check_form(e, name)
    _against(res, e.debug_gate()[0], ref)
    rres, rg = _resident(e, half)
    _against(rres, rg, ref)


@pytest.mark.parametrize("name", list(wr.SHAPES))
def test_heterogeneous_weights_equal_the_restatement(name):
    """sigma_v = sigma 2^k, k per view from {-1, 0, 1, 2}.  The one-shot and the resident path agree bit for bit; the tracks in
    a shuffled caller order (the device brings the weights into the pipeline's order with them) give each track the same
    gamma and the batch the same update."""
    e, prob, ref = _engine(name), _problem(name), _het_ref(name)
    het = _with(prob, _het(name))
    res = e.update_problem(het)
    g = e.debug_gate()[0]
    _check_form(e, name)
    _against(res, g, ref)
    plain = e.update_problem(prob)
    assert not np.array_equal(plain.dx, res.dx)                # (the weights did something)
    rres, rg = _resident(e, het)
    assert _same(rres, res) and np.array_equal(rg, g)
    perm = np.random.default_rng(5).permutation(prob.F)
    shuffled = het.take(perm)
    sres = e.update_problem(shuffled)
    sg = e.debug_gate()[0]
    assert sres.status == 0 and np.array_equal(sres.accepted, res.accepted[perm])
    assert np.array_equal(sg, g[perm])
    assert rel_err(sres.dx, ref["dx"]) < TOL and rel_err(sres.P_new, ref["P_new"]) < TOL
    e.load(shuffled)
    e.run()
    assert _same(e.result(), sres) and np.array_equal(e.debug_gate()[0], sg)


def test_selection_then_run_honours_the_weights():
    """run_select + run on the band shape with weights == the restatement on the valid subset with the refreshed points."""
    name = "band"
    e, prob = _engine(name), _problem(name)
    het = _with(prob, _het(name))
    tracks = synth.make_tracks(prob, wr.shape_seed(name), lost_fraction=0.6)
    params = synth.SelectParams(min_parallax_deg=8.0)
    exp = oracle.select_features(prob, tracks, params)
    valid = np.nonzero(exp["flags"] & 1)[0]
    assert 0 < valid.size < prob.F
    chained = het.take(valid)
    chained.idp_m, chained.idp_rho = exp["idp_m"][valid], exp["idp_rho"][valid]
    ref = wr.update(chained)
    assert ref["status"] == 0 and wr.clear_of_threshold(ref)
    e.load(het)
    e.set_tracks(tracks)
    e.run_select(params, prob.K)
    e.run()
    res = e.result()
    assert np.array_equal(e.selection().flags & 1, exp["flags"] & 1)
    assert res.status == 0 and np.array_equal(res.accepted[valid], ref["accepted"]) and res.n_rejected == ref["n_rejected"]
    assert np.allclose(e.debug_gate()[0][valid], ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
    e.replan()                                                  # the plan over the valid tracks only: the same update
    e.run()
    again = e.result()
    assert np.array_equal(again.accepted, res.accepted)
    assert rel_err(again.dx, ref["dx"]) < TOL and rel_err(again.P_new, ref["P_new"]) < TOL


def _code(fn, *a):
    with pytest.raises(_ffi.EngineError) as ei:
        fn(*a)
    return ei.value.code


def test_lifetime_and_errors():
    from msckf_amd.api import UpdateEngine
    name = "band"
    prob, vs = _problem(name), _het(name)
    N, F, M, _, plan = wr.SHAPES[name]
    with UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan) as e:
        assert _code(e.set_view_sigma, vs) == _ffi.ERR_STATE   # before any batch
        assert _code(e.set_view_sigma, None) == _ffi.ERR_STATE
        e.set_state(prob)
        assert _code(e.set_view_sigma, vs) == _ffi.ERR_STATE   # a state, no batch
        plain, pg = _resident(e, prob)
        e.set_view_sigma(vs)
        e.run()
        het, hg = e.result(), e.debug_gate()[0]
        assert not np.array_equal(het.dx, plain.dx)
        _against(het, hg, _het_ref(name))
        # a bad entry: MSCKF_ERR_ARG, and the weights in force stay
        for bad in (np.nan, np.inf, 0.0, -0.2):
            v = np.array(vs)
            v[v.size // 2] = bad
            assert _code(e.set_view_sigma, v) == _ffi.ERR_ARG
            e.run()
            assert _same(e.result(), het) and np.array_equal(e.debug_gate()[0], hg)
        with pytest.raises(ValueError):
            e.set_view_sigma(vs[:-1])
        # NULL clears
        e.set_view_sigma(None)
        e.run()
        assert _same(e.result(), plain) and np.array_equal(e.debug_gate()[0], pg)
        # ... so does a new batch
        e.set_view_sigma(vs)
        e.set_features(prob)
        e.run()
        assert _same(e.result(), plain)
        # ... and a new state (w_v was taken at the sigma it replaces)
        e.set_view_sigma(vs)
        e.set_state(prob)
        e.run()
        assert _same(e.result(), plain)
        # run_timed and run_compress go through the same K1
        e.set_view_sigma(vs)
        e.run_timed(2)
        assert _same(e.result(), het)
        # the one-shot call brings its own weights or none
        assert _same(e.update_problem(prob), e.update_problem(_with(prob, None)))
        bad = np.array(vs)
        bad[0] = -1.0
        assert _code(e.update_problem, _with(prob, bad)) == _ffi.ERR_ARG
        assert _same(e.update_problem(_with(prob, vs)), e.update_problem(_with(prob, vs)))


@pytest.mark.parametrize("name", ["band", "split"])
def test_heterogeneous_weights_on_an_f32_stack(name):
    e, prob = _engine(name, "f32"), _problem(name)
    res = e.update_problem(_with(prob, _het(name)))
    assert (e.debug_split()["long_tracks"] > 0) == FORMS[name][2]
    _against(res, e.debug_gate()[0], _het_ref(name), TOL32_DX, TOL32_P)
    rres, rg = _resident(e, _with(prob, _het(name)))
    _against(rres, rg, _het_ref(name), TOL32_DX, TOL32_P)


def test_two_logical_shards_carry_their_own_weights():
    """The band shape as 2 shards on one GPU: each loads its tracks with its slice of the weights, exports its group
    triangles, the root merges -- the records and the merge know nothing of the weights."""
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import partition_features
    name = "band"
    prob, ref = _problem(name), _het_ref(name)
    het = _with(prob, _het(name))
    N, F, M, _, plan = wr.SHAPES[name]
    with UpdateEngine(max_clones=N, max_features=F, max_track=M, plan=plan) as e:
        assert e.band_ok(prob)
        e.set_group_exchange(True)
        recs, total, acc = [], 0, np.zeros(prob.F, dtype=np.uint8)
        shards = partition_features(prob.view_ptr, 2)
        assert all(hi > lo for lo, hi in shards)
        for lo, hi in shards:
            local = het.subset(lo, hi)
            assert np.array_equal(local.view_sigma, het.view_sigma[prob.view_ptr[lo]:prob.view_ptr[hi]])
            e.load(local)
            e.run_compress()
            rec, n = e.export_groups()
            acc[lo:hi] = e.result().accepted
            recs.append(rec); total += n
        e.set_state(prob)
        e.merge_groups(np.stack(recs), total)
        res = e.result()
        assert res.status == 0 and np.array_equal(acc, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL


def test_store_batch_takes_weights_in_its_view_order():
    """A batch of the track store (tracks_observe ... load_tracks_where) with set_view_sigma in the batch's view order equals,
    bit for bit, the same batch through set_features + set_view_sigma on a second engine."""
    from msckf_amd.api import UpdateEngine
    from test_gpu_tracks import _grow, _small, _store_batch
    p, uv = _small(6, 10, seed=11)
    ids = [3, 14, 15, 9, 26, 5, 35, 8, 97, 12]
    views = [[0, 1, 2, 3, 4, 5], [0, 2, 3, 5], [1, 2, 3], [2, 3, 4, 5], [0, 1, 2, 3, 4], [3, 4, 5], [0, 1, 4, 5], [1, 2, 3, 4, 5],
             [0, 5], [2, 3, 4]]
    # (observe keeps no frame counters: no track is lost, every one has parallax and is triangulated afresh)
    params = synth.SelectParams(min_frames_lost=1, min_frames_tracked=2, use_parallax=True, min_parallax_deg=0.0)
    kw = dict(max_clones=8, max_features=16, max_track=8)
    with UpdateEngine(**kw) as eng, UpdateEngine(**kw) as eng_b:
        _grow(eng, p, uv, views, ids)
        P = eng.covariance()
        order = eng.load_tracks_where()
        assert sorted(order.tolist()) == sorted(ids)
        n = sum(map(len, views))
        vs = p.sigma * np.exp2(np.random.default_rng(7).choice(np.array(wr.HET_POWERS), size=n).astype(np.float64))

        def finish(e):
            e.run_select(params, p.K)
            sel = e.selection()
            e.run()
            return sel, e.result(), e.debug_gate()[0]
        plain = finish(eng)
        _, b = _store_batch(eng, order)                         # (the rows as the selection's refresh left them)
        assert int(b["view_ptr"][-1]) == n
        assert np.array_equal(eng.load_tracks_where(), order)
        eng.set_view_sigma(vs)
        sel, res, g = finish(eng)
        assert sel.valid.all() and res.status == 0 and not np.array_equal(res.dx, plain[1].dx)
        # the same batch through the host's door
        eng_b.set_prior(P, p.gravity, p.K, p.sigma, p.cam_R, p.cam_t)
        prob = synth.UpdateProblem(P=P, cam_R=p.cam_R, cam_t=p.cam_t, cam_R0=p.cam_R, cam_t0=p.cam_t, gravity=p.gravity, K=p.K,
                                   sigma=p.sigma, view_ptr=b["view_ptr"], obs_uv=b["obs_uv"], obs_slot=b["obs_slot"],
                                   idp_base=b["idp_base"], idp_m=b["idp_m"].copy(), idp_rho=b["idp_rho"].copy())
        eng_b.set_features(prob)
        eng_b.set_view_sigma(vs)
        lost, tracked = eng.tracks_counters(order)
        eng_b.set_tracks(synth.TrackTable(line_base=b["line_base"], line_dir=b["line_dir"], line_conf=b["line_conf"],
                                          lost_for=lost, tracked_for=tracked))
        sel_b, res_b, g_b = finish(eng_b)
        assert np.array_equal(sel.flags, sel_b.flags) and np.array_equal(sel.idp_m, sel_b.idp_m)
        assert _same(res, res_b) and np.array_equal(g, g_b)


def test_reference_shaped_adapter_takes_a_mapping():
    """`update(filt, features, view_sigma={key: per-view sigmas})`: packed in the order of `Feature.keypoints`, the covariance
    the filter is left with is the restatement's; features the mapping does not name stay at sigma_image."""
    from conftest import load_golden
    from msckf_amd.api import UpdateEngine
    from test_host_logic import make_reference_shaped
    prob, gold = load_golden("edge_some_rejected")
    filt, feats = make_reference_shaped(prob, gold)
    keys = list(feats)
    rng = np.random.default_rng(3)
    mapping = {k: prob.sigma * np.exp2(rng.choice(np.array(wr.HET_POWERS), size=len(feats[k].keypoints)).astype(np.float64))
               for k in keys[::2]}
    vs = np.concatenate([mapping.get(k, np.full(len(feats[k].keypoints), prob.sigma)) for k in keys])
    ref = wr.update(prob, vs)
    assert ref["status"] == 0 and wr.clear_of_threshold(ref) and 0 < ref["n_rejected"] < prob.F
    M = int(np.diff(prob.view_ptr).max())
    with UpdateEngine(max_clones=prob.N, max_features=prob.F, max_track=max(M, 2)) as e:
        assert e.update(filt, feats, view_sigma=mapping) == 0
        assert np.allclose(e.debug_gate()[0], ref["gamma"], rtol=GAMMA_RTOL, atol=0.0)
    assert filt.number_of_residuals_discarded_for_gasting_test == ref["n_rejected"]
    assert rel_err(filt.state.covariance, ref["P_new"]) < TOL
