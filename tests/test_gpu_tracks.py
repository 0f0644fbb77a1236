"""The resident track store: `tracks_observe` / `load_tracks` / `tracks_remove` and `remove_clones` on a store.

2  The reference's 30-clone run (`golden/window30/seq_window30.npz`) on a nominal-resident engine whose batches come from
   the store: only the frame's keypoints travel (`track_events.py`), `nominal()` is called to check, never to feed.
   Store contents at every call's entry against the fixture; flags, masks, status, counters exact; dx, probes and
   checkpoints 1e-8 relative; bookkeeping after every call.
3  The same batch through both doors, bit for bit: at a short-track call, one with split long tracks and a prune call the
   store's arrays (`track(id)`) go to a second engine with the same state through `set_features` + `set_tracks`.
4  Small hand-built cases: ragged tracks and the removal of a middle clone, a 31-view track, subsets in permuted order,
   error codes, `tracks_reset` / `set_state`, an empty `load_tracks`.

Worst errors on one MI355X, steps 2 and 3: see DESIGN.md 3.8."""
import numpy as np
import pytest

from conftest import rel_err
import nominal_ref
import track_events
import window30
from window30 import AUGMENT, PROCESS, PRUNE, REMOVE
from test_gpu_select import EPS

pytestmark = pytest.mark.gpu

TOL = 1e-8
POSE_TOL = 1e-9
F64EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def run():
    return window30.Run()


@pytest.fixture(scope="module")
def events(run):
    return track_events.derive(run)


def _engine(dtype=None, **kw):
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=31, max_features=512, max_track=31, dtype=dtype or "f64")
    args.update(kw)
    return UpdateEngine(**args)


def _store_batch(eng, ids):
    """The candidates as the store holds them, in the layout of `set_features` + `set_tracks`."""
    tr = [eng.track(int(i)) for i in ids]
    nv = [len(t["slots"]) for t in tr]
    cat = lambda k, w: np.concatenate([t[k].reshape(-1, w) for t in tr]) if tr else np.zeros((0, w))
    return tr, dict(view_ptr=np.concatenate([[0], np.cumsum(nv)]).astype(np.int32), obs_uv=cat("uv", 2),
                    obs_slot=np.concatenate([t["slots"] for t in tr]).astype(np.int32) if tr else np.zeros(0, np.int32),
                    line_base=cat("line_base", 3), line_dir=cat("dir", 3), line_conf=cat("conf", 1).reshape(-1),
                    idp_base=np.array([t["idp_base"] for t in tr]).reshape(-1, 3),
                    idp_m=np.array([t["idp_m"] for t in tr]).reshape(-1, 3), idp_rho=np.array([t["idp_rho"] for t in tr]))


def _host_door(eng_b, b, P, cam_R, cam_t, gravity, K, sigma, lost, tracked, params):
    """The batch `b` through `set_features` + `set_tracks` on a second engine holding the same state."""
    from msckf_amd import synth
    eng_b.set_prior(P, gravity, K, sigma, cam_R, cam_t)
    prob = synth.UpdateProblem(P=P, cam_R=cam_R, cam_t=cam_t, cam_R0=cam_R, cam_t0=cam_t, gravity=gravity, K=K, sigma=sigma,
                               view_ptr=b["view_ptr"], obs_uv=b["obs_uv"], obs_slot=b["obs_slot"], idp_base=b["idp_base"],
                               idp_m=b["idp_m"].copy(), idp_rho=b["idp_rho"].copy())
    eng_b.set_features(prob)
    eng_b.set_tracks(synth.TrackTable(line_base=b["line_base"], line_dir=b["line_dir"], line_conf=b["line_conf"],
                                      lost_for=lost, tracked_for=tracked))
    eng_b.run_select(params, K)
    sel = eng_b.selection()
    n_valid = int(sel.valid.sum())
    if 0 < n_valid < 0.15 * prob.F:
        eng_b.replan()
    res = None
    if n_valid:
        eng_b.run()
        res = eng_b.result()
    return sel, res


def _same_through_both_doors(sel, res, sel_b, res_b, what):
    assert np.array_equal(sel.flags, sel_b.flags), what
    assert np.array_equal(sel.idp_m, sel_b.idp_m) and np.array_equal(sel.idp_rho, sel_b.idp_rho), what
    assert (res is None) == (res_b is None), what
    if res is not None:
        assert res.status == res_b.status and np.array_equal(res.accepted, res_b.accepted), what
        assert np.array_equal(res.dx, res_b.dx) and np.array_equal(res.P_new, res_b.P_new), what


def _drive(run, events, eng, check=True, doors=None, last_call=None):
    """The run with the tracks resident.  check: everything of step 2 against the fixture; doors: {call: second engine}
    for step 3.  Returns the worst errors and counters."""
    from oracle import msckf_oracle as oracle
    from msckf_amd import synth
    z = run.z
    params = run.select_params()
    Kinv = np.linalg.inv(z["K"])
    gyro, acc = nominal_ref.raw_samples(run)
    eng.set_prior(z["P0"], z["gravity"], z["K"], run.sigma)
    eng.set_nominal(z["imu_R0"][0], z["imu_t0"][0], z["imu_v0"][0], z["gravity"], z["Qc"],
                    T_W_I=(z["T_W_I_R"], z["T_W_I_t"]), T_W_C=(z["T_W_C_R"], z["T_W_C_t"]))
    keys = []
    w = dict(dx=0.0, probe=0.0, dir=0.0, base=0.0, m=0.0, rho=0.0, stale=0, updates=0, split_updates=0, doors=0)
    anchor_key, frozen, m_tol = {}, {}, {}
    assert eng.tracks_count() == (0, 0)
    for kind, idx, o in nominal_ref.imu_groups(run):
        if kind == "imu":
            eng.propagate_imu(gyro[idx], acc[idx], z["imu_dt"][idx])
            continue
        if kind == AUGMENT:
            eng.augment_imu()
            keys.append(int(run.aug(idx)["key"]))
            continue
        assert kind in (PROCESS, PRUNE)                              # (the run holds no REMOVE op, test_tracks_host.py)
        c, ev = run.call(idx), events[idx]
        N = len(keys)
        assert c["keys"].tolist() == keys and eng.n_clones == N
        # -- the frame's keypoints: all that travels
        pool = ev["observe_pool"]
        known = set(anchor_key)
        eng.tracks_observe(ev["observe_ids"], z["pool_uv"][pool].astype(np.float64), z["pool_score"][pool].astype(np.float64))
        fresh = [int(i) for i in ev["observe_ids"] if int(i) not in known]
        for i in fresh:
            anchor_key[i] = keys[-1]
        vp = c["view_ptr"]
        held = eng.nominal() if (check or (doors and idx in doors)) else None
        entry = None
        if check or (doors and idx in doors):
            tr, entry = _store_batch(eng, c["ids"])
        if check:
            # -- store contents at the call's entry
            assert np.array_equal(entry["view_ptr"], vp) and np.array_equal(entry["obs_slot"], c["obs_slot"])
            assert np.array_equal(entry["obs_uv"], c["obs_uv"]) and np.array_equal(entry["line_conf"], c["line_conf"])
            e = np.hstack([c["obs_uv"], np.ones((len(c["obs_uv"]), 1))]) @ Kinv.T
            d_err = np.abs(entry["line_dir"] - c["line_dir"]).max(axis=1)
            assert np.all(d_err <= POSE_TOL * np.abs(e).sum(axis=1) + 8 * F64EPS * np.linalg.norm(e, axis=1)), (idx, d_err.max())
            w["dir"] = max(w["dir"], float(d_err.max()))
            assert np.array_equal(entry["line_base"], held["cam_t"][c["obs_slot"]])
            b_err = float(np.abs(entry["line_base"] - c["line_base"]).max())
            assert b_err <= POSE_TOL, (idx, b_err)
            for j, (fid, t) in enumerate(zip(c["ids"].tolist(), tr)):
                if anchor_key[fid] in keys:
                    assert t["anchor_slot"] == keys.index(anchor_key[fid])
                    assert np.array_equal(t["idp_base"], held["cam_t"][t["anchor_slot"]]), (idx, fid)
                else:
                    assert t["anchor_slot"] == -1 and np.array_equal(t["idp_base"], frozen[fid]), (idx, fid)
                    w["stale"] += int(c["flags"][j] & 1)
                b_err = max(b_err, float(np.abs(t["idp_base"] - c["idp_base"][j]).max()))
                if fid in fresh:
                    assert t["idp_rho"] == 0.1
            assert b_err <= POSE_TOL, (idx, b_err)
            w["base"] = max(w["base"], b_err)
            # refreshed points were written back: the entry values are the fixture's, within what the refreshing call's
            # own check allowed (never refreshed: m = dir / |dir| against the reference's trigonometric form, 1e-12)
            pose = 3 * POSE_TOL * (1 + np.abs(c["idp_rho"]))
            tol0 = np.array([m_tol.get(fid, 1e-12) for fid in c["ids"].tolist()])
            m_err, r_err = np.abs(entry["idp_m"] - c["idp_m"]).max(axis=1), np.abs(entry["idp_rho"] - c["idp_rho"])
            assert np.all(m_err <= tol0 + pose) and np.all(r_err <= (tol0 + pose) * np.abs(c["idp_rho"])), (idx, m_err.max(), r_err.max())
            w["m"], w["rho"] = max(w["m"], float(m_err.max())), max(w["rho"], float((r_err / np.abs(c["idp_rho"])).max()))
        door = None
        if doors and idx in doors:
            door = _host_door(doors[idx], entry, eng.covariance(), held["cam_R"], held["cam_t"], z["gravity"], z["K"], run.sigma,
                              c["lost"], c["tracked"], params)
        # -- the batch, by id
        eng.load_tracks(c["ids"], c["lost"], c["tracked"])
        eng.run_select(params, z["K"])
        sel = eng.selection()
        if check:
            prob = run.problem(c, np.zeros((15 + 6 * N,) * 2), held["cam_R"], held["cam_t"])
            cond = oracle.select_features(prob, run.tracks(c), params)["cond"]
            assert np.array_equal(sel.flags, c["flags"]), idx
            tol = np.minimum(np.maximum(200 * EPS * cond, 1e-12), TOL)
            ref = (c["flags"] & 4) > 0
            pose = 3 * POSE_TOL * (1 + np.abs(c["sel_rho"]))
            assert np.all(np.abs(sel.idp_rho - c["sel_rho"])[ref] <= ((tol + pose) * np.abs(c["sel_rho"]))[ref]), idx
            assert np.all(np.abs(sel.idp_m - c["sel_m"]).max(axis=1)[ref] <= (tol + pose)[ref]), idx
            scale = np.maximum(np.linalg.norm(c["world"][ref], axis=1), 1.0)
            assert np.all(np.linalg.norm(sel.world[ref] - c["world"][ref], axis=1) <= tol[ref] * scale), idx
            assert np.array_equal(sel.idp_m[~ref], entry["idp_m"][~ref]) and np.array_equal(sel.idp_rho[~ref], entry["idp_rho"][~ref])
            for j in np.nonzero(ref)[0]:
                m_tol[int(c["ids"][j])] = float(tol[j])
        n_valid = int(sel.valid.sum())
        if 0 < n_valid < 0.15 * len(c["ids"]):
            eng.replan()
        res = None
        if n_valid:
            eng.run()
            res = eng.result()
            if check:
                assert res.status == c["status"] and res.n_rejected == c["n_rejected"], idx
                assert np.array_equal(res.accepted, c["accepted"]), idx
            if res.status == 0:
                w["updates"] += 1
                w["split_updates"] += int(eng.debug_split()["long_tracks"] > 0)
                if check:
                    e = rel_err(res.dx, c["dx"])
                    w["dx"] = max(w["dx"], e)
                    assert e < TOL, (idx, e)
            assert eng.commit_inject() == res.status
        elif check:
            assert c["status"] == 1
        if door is not None:
            _same_through_both_doors(sel, res, door[0], door[1], idx)
            w["doors"] += 1
            w["door_split_%d" % idx] = int(res is not None and eng.debug_split()["long_tracks"] > 0)
        # -- what leaves
        eng.tracks_remove(ev["remove"])
        if len(ev["rm"]):
            before = eng.nominal()["cam_t"]                          # the rows as they stand just before the removal
            gone = {keys[s]: before[s].copy() for s in ev["rm"]}
            for fid, k in anchor_key.items():
                if k in gone and fid not in frozen:
                    frozen[fid] = gone[k]
            eng.remove_clones(ev["rm"])
            keys = [k for s, k in enumerate(keys) if s not in ev["rm"]]
            assert sorted(eng.tracks_dropped().tolist()) == ev["dropped"], idx
        assert eng.tracks_count() == (len(c["exit_ids"]), int(c["exit_nview"].sum())), idx
        if check:
            s = eng.nominal()
            assert float(np.abs(s["cam_R"] - c["post_R"]).max()) <= POSE_TOL and float(np.abs(s["cam_t"] - c["post_t"]).max()) <= POSE_TOL, idx
            P = None
            if o in run.probes or o in run.checkpoints:
                P = eng.covariance()
                assert np.array_equal(P, P.T), o
            for ref_v, got in ((run.probes.get(o), lambda: P @ run.V[:P.shape[0]]), (run.checkpoints.get(o), lambda: P)):
                if ref_v is not None:
                    e = rel_err(got(), ref_v)
                    w["probe"] = max(w["probe"], e)
                    assert e < TOL, (o, e)
        if last_call is not None and idx >= last_call:
            break
    return w


# ---- 2: the 30-clone run with the tracks resident ---------------------------------------------------------------------
def test_window30_run_with_the_tracks_resident(run, events):
    with _engine() as eng:
        w = _drive(run, events, eng)
    print(f"tracks window30: {w['updates']} updates, {w['split_updates']} with split long tracks, {w['stale']} stale-anchor "
          f"selections; worst dx {w['dx']:.2e}, probes {w['probe']:.2e}, dir {w['dir']:.2e}, bases {w['base']:.2e}, "
          f"entry m {w['m']:.2e}, entry rho {w['rho']:.2e}")
    assert w["stale"] >= 1 and w["split_updates"] >= 10, w


# ---- 3: the same batch through both doors -------------------------------------------------------------------------------
def _door_calls(run):
    """A short-track call, one whose update splits long tracks, a prune call with an update."""
    short = split = prune = None
    for i in range(run.n_calls()):
        c = run.call(i)
        if c["status"] != 0:
            continue
        vp, valid = c["view_ptr"], np.nonzero(c["flags"] & 1)[0]
        span = max(int(c["obs_slot"][vp[j + 1] - 1] - c["obs_slot"][vp[j]] + 1) for j in valid)
        if c["kind"] == PROCESS and span <= 10 and short is None:
            short = i
        if c["kind"] == PROCESS and span > window30.SPLIT_SPAN and split is None:
            split = i
        if c["kind"] == PRUNE and prune is None:
            prune = i
    assert None not in (short, split, prune)
    return short, split, prune


def test_store_batch_equals_the_host_batch_bit_for_bit(run, events):
    short, split, prune = _door_calls(run)
    with _engine() as eng, _engine() as eng_b:
        w = _drive(run, events, eng, check=False, doors={short: eng_b, split: eng_b, prune: eng_b}, last_call=max(short, split, prune))
    assert w["doors"] == 3 and w["door_split_%d" % split] == 1 and w["door_split_%d" % short] == 0, w


def test_store_batch_equals_the_host_batch_on_f32_engines(run, events):
    short, _, _ = _door_calls(run)
    with _engine("f32") as eng, _engine("f32") as eng_b:
        w = _drive(run, events, eng, check=False, doors={short: eng_b}, last_call=short)
    assert w["doors"] == 1, w


# ---- 4: small hand-built cases ---------------------------------------------------------------------------------------------
J15 = np.zeros((6, 15))
J15[0:3, 0:3] = np.eye(3)
J15[3:6, 12:15] = np.eye(3)


def _small(N, F, seed):
    """Synthetic poses and consistent keypoints: feature j's view in clone s is uv[j, s]."""
    from msckf_amd import synth
    p = synth.make_problem(N, F, N, seed=seed)
    assert np.array_equal(np.asarray(p.obs_slot).reshape(F, N), np.tile(np.arange(N), (F, 1)))
    return p, np.asarray(p.obs_uv, dtype=np.float64).reshape(F, N, 2)


def _grow(eng, p, uv, views, ids):
    """One clone at a time: `views[j]` lists the clones track ids[j] is seen in."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((15, 15))
    eng.set_prior(A @ A.T / 15 + np.eye(15) * 0.1, p.gravity, p.K, p.sigma)
    for s in range(p.N):
        eng.augment(J15, p.cam_R[s], p.cam_t[s])
        js = [j for j in range(len(ids)) if s in views[j]]
        eng.tracks_observe([ids[j] for j in js], uv[js, s], 0.5 + 0.01 * np.arange(len(js)))


def _snapshot(eng, ids):
    return eng.tracks_count(), [eng.track(i) for i in ids]


def _same_snapshot(a, b):
    return a[0] == b[0] and all(np.array_equal(x[k], y[k]) for x, y in zip(a[1], b[1]) for k in x)


PARAMS = dict(min_frames_lost=1, min_frames_tracked=2, use_parallax=False, min_parallax_deg=0.0)


def test_ragged_tracks_and_the_removal_of_a_middle_clone():
    from msckf_amd import synth
    p, uv = _small(4, 6, seed=5)
    ids = [11, 3, 7, 20, 5, 9]
    views = [[0, 1, 2, 3], [0, 2, 3], [1], [1, 2], [2, 3], [0, 1]]      # 3: skips clone 1; 7: only the clone that goes
    with _engine(max_clones=8, max_features=8, max_track=6) as eng:
        _grow(eng, p, uv, views, ids)
        assert eng.tracks_count() == (6, sum(map(len, views)))
        Kinv = np.linalg.inv(p.K)
        for j, i in enumerate(ids):
            t = eng.track(i)
            assert t["slots"].tolist() == views[j] and t["anchor_slot"] == views[j][0] and t["idp_rho"] == 0.1
            assert np.array_equal(t["uv"], uv[j, views[j]]) and np.array_equal(t["line_base"], p.cam_t[views[j]])
            assert np.array_equal(t["idp_base"], p.cam_t[views[j][0]])
            d = np.array([p.cam_R[s] @ (Kinv @ np.append(uv[j, s], 1)) for s in views[j]])
            assert np.abs(t["dir"] - d).max() <= 8 * F64EPS * np.abs(d).max()
            assert np.abs(t["idp_m"] - d[0] / np.linalg.norm(d[0])).max() <= 4 * F64EPS
        before = {i: eng.track(i) for i in ids}
        eng.remove_clones([1])
        assert eng.tracks_dropped().tolist() == [7] and eng.tracks_count() == (5, 10)
        remap = {0: 0, 2: 1, 3: 2}
        keep = [0, 2, 3]
        for j, i in enumerate(ids):
            if i == 7:
                continue
            t, b = eng.track(i), before[i]
            sel = [k for k, s in enumerate(views[j]) if s != 1]
            assert t["slots"].tolist() == [remap[views[j][k]] for k in sel]
            for k in ("uv", "dir", "conf"):
                assert np.array_equal(t[k], b[k][sel]), (i, k)
            assert np.array_equal(t["line_base"], p.cam_t[keep][t["slots"]])
            if views[j][0] == 1:                                     # 20: its anchor went
                assert t["anchor_slot"] == -1 and np.array_equal(t["idp_base"], p.cam_t[1])
            else:
                assert t["anchor_slot"] == remap[views[j][0]] and np.array_equal(t["idp_base"], p.cam_t[views[j][0]])
            assert np.array_equal(t["idp_m"], b["idp_m"]) and t["idp_rho"] == b["idp_rho"]
        moved_R, moved_t = p.cam_R[keep], p.cam_t[keep] + np.array([0.25, -0.5, 0.125])
        eng.set_poses(moved_R, moved_t)
        for j, i in enumerate(ids):
            if i == 7:
                continue
            t = eng.track(i)
            assert np.array_equal(t["line_base"], moved_t[t["slots"]])
            assert np.array_equal(t["idp_base"], p.cam_t[1] if i == 20 else moved_t[t["anchor_slot"]])
        # the batch the emit kernel writes carries the same bases
        eng.load_tracks([20, 11], [1, 1], [2, 3])
        eng.run_select(synth.SelectParams(**PARAMS), p.K)
        assert eng.selection().flags.shape == (2,)
        with pytest.raises(Exception):
            eng.track(7)


def test_a_track_of_31_views_equals_the_host_batch():
    from msckf_amd import synth
    p, uv = _small(31, 5, seed=9)
    ids = [4, 8, 15, 16, 23]
    views = [list(range(31)), list(range(0, 31, 3)), list(range(20, 31)), [0, 30], list(range(5, 17))]
    params = synth.SelectParams(**PARAMS)
    with _engine(max_features=16) as eng, _engine(max_features=16) as eng_b:
        _grow(eng, p, uv, views, ids)
        assert len(eng.track(4)["slots"]) == 31 and eng.tracks_count() == (5, sum(map(len, views)))
        lost, tracked = np.ones(5, np.int32), np.array([len(v) for v in views], np.int32)
        _, b = _store_batch(eng, ids)
        door = _host_door(eng_b, b, eng.covariance(), p.cam_R, p.cam_t, p.gravity, p.K, p.sigma, lost, tracked, params)
        eng.load_tracks(ids, lost, tracked)
        eng.run_select(params, p.K)
        sel = eng.selection()
        assert sel.valid.all() and (sel.flags & 4).any()
        eng.run()
        res = eng.result()
        assert res.status == 0 and eng.debug_split()["long_tracks"] > 0
        _same_through_both_doors(sel, res, door[0], door[1], "31 views")
        # the refreshed points went back to the rows
        for j, i in enumerate(ids):
            t = eng.track(i)
            assert np.array_equal(t["idp_m"], sel.idp_m[j]) and t["idp_rho"] == sel.idp_rho[j]


def test_a_subset_in_permuted_order_follows_the_given_order():
    from msckf_amd import synth
    p, uv = _small(4, 6, seed=6)
    ids = [1, 2, 3, 4, 5, 6]
    views = [[0, 1, 2, 3], [0, 1, 2], [1, 2, 3], [2, 3], [0, 1, 2, 3], [3]]
    params = synth.SelectParams(**PARAMS)
    with _engine(max_clones=8, max_features=8, max_track=6) as eng:
        _grow(eng, p, uv, views, ids)
        out = {}
        for order in ([5, 1, 6, 3], [3, 6, 1, 5]):
            lost = np.array([0 if i == 6 else 1 for i in order], np.int32)     # 6 is not lost and has one view: not valid
            eng.load_tracks(order, lost, np.full(4, 3, np.int32))
            eng.run_select(params, p.K)
            sel = eng.selection()
            assert [bool(v) for v in sel.valid] == [i != 6 for i in order]
            eng.run()
            res = eng.result()
            out[tuple(order)] = {i: (int(sel.flags[k]), int(res.accepted[k])) for k, i in enumerate(order)}
            assert res.accepted[order.index(6)] == 0
            # (no commit: the second order starts from the same prior, and the selection refreshes the same points again)
        assert out[(5, 1, 6, 3)] == out[(3, 6, 1, 5)]


def test_error_codes_leave_the_store_as_it_was():
    from msckf_amd import _ffi
    p, uv = _small(3, 5, seed=7)
    ids = [1, 2, 3, 4]
    views = [[0, 1, 2], [0, 1], [1, 2], [0, 1, 2]]

    def code(fn, *a):
        with pytest.raises(_ffi.EngineError) as err:
            fn(*a)
        return err.value.code

    with _engine(max_clones=4, max_features=5, max_track=3) as eng:
        with pytest.raises(_ffi.EngineError):                        # no state yet
            eng.tracks_observe([1], uv[0, :1], [1.0])
        eng.set_prior(np.eye(15), p.gravity, p.K, p.sigma)
        assert code(eng.tracks_observe, [1], uv[0, :1], [1.0]) == _ffi.ERR_STATE     # N = 0
        _grow(eng, p, uv, views, ids)
        snap = _snapshot(eng, ids)
        one = uv[0, 2:3]
        assert code(eng.tracks_observe, [1], one, [1.0]) == _ffi.ERR_DUP_SLOT        # already seen in the newest clone
        assert code(eng.tracks_observe, [2, 2], uv[1, 1:3], [1.0, 1.0]) == _ffi.ERR_DUP_SLOT
        assert code(eng.tracks_observe, [8, 9], uv[1, 1:3], [1.0, 1.0]) == _ffi.ERR_ARG   # five rows, four in use
        assert code(eng.tracks_remove, [2, 77]) == _ffi.ERR_ARG
        assert code(eng.load_tracks, [1, 77], [1, 1], [2, 2]) == _ffi.ERR_ARG
        assert code(eng.load_tracks, [1, 1], [1, 1], [2, 2]) == _ffi.ERR_ARG
        assert _same_snapshot(snap, _snapshot(eng, ids))
        eng.augment(J15, p.cam_R[2], p.cam_t[2] + 1.0)               # a fourth clone: track 1 holds max_track views already
        assert code(eng.tracks_observe, [2, 1], uv[1, 1:3], [1.0, 1.0]) == _ffi.ERR_ARG
        assert _same_snapshot(snap, _snapshot(eng, ids))
        eng.tracks_observe([2], one, [0.75])                         # ... and the store still works
        assert eng.track(2)["slots"].tolist() == [0, 1, 3] and eng.tracks_count() == (4, 11)


def test_reset_set_state_and_an_empty_load():
    from msckf_amd import _ffi, synth
    p, uv = _small(3, 4, seed=8)
    ids = [1, 2, 3, 4]
    views = [[0, 1, 2], [0, 1], [1, 2], [2]]
    with _engine(max_clones=4, max_features=8, max_track=4) as eng:
        _grow(eng, p, uv, views, ids)
        assert eng.tracks_count() == (4, 8)
        eng.tracks_reset()
        assert eng.tracks_count() == (0, 0)
        with pytest.raises(_ffi.EngineError):
            eng.track(1)
        _grow(eng, p, uv, views, ids)                                # (set_prior -> msckf_set_state: empties it too)
        assert eng.tracks_count() == (4, 8)
        eng.set_state(p)
        assert eng.tracks_count() == (0, 0)
        eng.load_tracks([], [], [])                                  # as set_features(F = 0)
        eng.run_select(synth.SelectParams(**PARAMS), p.K)
        eng.run()
        res = eng.result()
        assert res.status == 1 and not res.dx.any() and res.accepted.size == 0
        assert np.array_equal(res.P_new, np.asarray(p.P))
