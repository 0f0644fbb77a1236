"""Frame intake on the resident track store: `tracks_frame`, `load_tracks_where`, `tracks_counters`, `tracks_clone_views`.

1  The reference's own `add_camera_measurements` (`golden/assoc_tests.npz`) with the tracks in the store: appended views,
   both rejection counters, `lost_for` of all 160 tracks (the unmatched ones through `MSCKF.py:438`), `tracked_for`.
2  Results and failing views against `oracle.associate` and `associate` on the host batch, element for element, on 300
   tracks of 1-31 views (`frame_cases.py`: the inputs are first shown not to be thin).
3  The store afterwards is the store `tracks_observe` of the passing + fresh subset makes, bit for bit.
4  The reference's 30-clone run with no track integer on the host: candidates, their order and counters come from the store.
5  Hand-built cases: creation order over recycled rows, candidates by clone slot, counters over holes, a failing match, the
   resident pose, error codes, per-clone view counts."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
import frame_cases
import nominal_ref
import track_events
import window30
from window30 import AUGMENT, PROCESS, PRUNE

pytestmark = pytest.mark.gpu

TOL = 1e-8
INF = float("inf")


def _engine(**kw):
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=32, max_features=512, max_track=32)
    args.update(kw)
    return UpdateEngine(**args)


# ---- 1: the reference's fixture through the store ----------------------------------------------------------------------
def test_reference_fixture_through_the_store():
    prob, z = load_golden("assoc_tests")
    ids = 100 + np.arange(prob.F)
    matched = ~np.isnan(z["assoc_matched_uv"][:, 0])
    with _engine(max_clones=9, max_features=prob.F, max_track=8) as eng:
        frame_cases.grow_store(eng, prob, ids)
        lost0, tracked0 = eng.tracks_counters(ids)
        assert not lost0.any() and np.array_equal(tracked0, np.diff(prob.view_ptr))
        eng.augment(frame_cases.J15, z["assoc_R_cur"], z["assoc_t_cur"])
        res, fail = eng.tracks_frame(ids[matched], z["assoc_matched_uv"][matched], np.ones(int(matched.sum())), prob.K,
                                     float(z["assoc_thr"][0]), float(z["assoc_thr"][1]))
        kept = np.zeros(prob.F, np.uint8)
        kept[matched] = res == 0
        assert np.array_equal(kept, z["assoc_kept"])
        assert int((res == 1).sum()) == int(z["assoc_n_epipolar"]) and int((res == 2).sum()) == int(z["assoc_n_homography"])
        assert np.array_equal((fail >= 0), res > 0)
        lost, tracked = eng.tracks_counters(ids)
        assert np.array_equal(lost, z["assoc_lost_for"])
        assert np.array_equal(tracked, np.diff(prob.view_ptr) + z["assoc_kept"])
        assert eng.tracks_count() == (prob.F, int(prob.view_ptr[-1]) + int(kept.sum()))


# ---- 2, 3: against msckf_run_associate and the oracle; the store afterwards ---------------------------------------------
@pytest.fixture(scope="module")
def case():
    from oracle import msckf_oracle as oracle
    prob, R_cur, t_cur, muv, score = frame_cases.assoc_case()
    outs = [oracle.associate(prob, muv, R_cur, t_cur, prob.K, te, th) for te, th in frame_cases.PAIRS]
    frame_cases.assert_not_thin(prob, outs)
    return dict(prob=prob, R_cur=R_cur, t_cur=t_cur, muv=muv, score=score, outs=outs)


def _fresh_pairs(rng, n):
    return 1000 + np.arange(n), np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)]), rng.uniform(0.2, 1.0, n)


@pytest.mark.parametrize("pair", [0, 1])
def test_results_equal_the_oracle_and_the_host_batch_and_the_store_is_observes(case, pair):
    prob, muv, score = case["prob"], case["muv"], case["score"]
    thr_e, thr_h = frame_cases.PAIRS[pair]
    ref, rfail = case["outs"][pair]
    ids = np.arange(prob.F) * 3 + 5
    view_score = np.random.default_rng(11).uniform(0.2, 1.0, int(prob.view_ptr[-1]))
    # three fresh pairs ride along: 303 pairs are 38 blocks of eight groups, the last one with an empty group
    f_ids, f_uv, f_score = _fresh_pairs(np.random.default_rng(12), 3)
    order = np.random.default_rng(13).permutation(prob.F + 3)
    all_ids = np.concatenate([ids, f_ids])[order]
    all_uv = np.concatenate([muv, f_uv])[order]
    all_score = np.concatenate([score, f_score])[order]
    with _engine() as a, _engine(max_clones=31, max_track=31) as b, _engine() as c:
        for eng in (a, c):
            frame_cases.grow_store(eng, prob, ids, view_score)
            eng.augment(frame_cases.J15, case["R_cur"], case["t_cur"])
        res, fail = a.tracks_frame(all_ids, all_uv, all_score, prob.K, thr_e, thr_h)
        back = np.argsort(order)
        res_t, fail_t = res[back][:prob.F], fail[back][:prob.F]
        assert np.array_equal(res[back][prob.F:], [4] * 3) and np.array_equal(fail[back][prob.F:], [-1] * 3)
        assert np.array_equal(res_t, ref) and np.array_equal(fail_t, rfail)
        b.load(prob)
        res_b, fail_b = b.associate(muv, case["R_cur"], case["t_cur"], prob.K, thr_e, thr_h)
        assert np.array_equal(res_t, res_b) and np.array_equal(fail_t, fail_b)
        # 3: the store is what tracks_observe of the passing + fresh subset makes
        keep = (res == 0) | (res == 4)
        c.tracks_observe(all_ids[keep], all_uv[keep], all_score[keep])
        assert a.tracks_count() == c.tracks_count()
        for i in all_ids.tolist():
            ta, tc = a.track(i), c.track(i)
            assert all(np.array_equal(ta[k], tc[k]) for k in ta), i
        nv = np.diff(prob.view_ptr)
        lost, tracked = a.tracks_counters(ids)
        assert np.array_equal(lost, (ref > 0).astype(np.int32)) and np.array_equal(tracked, nv + (ref == 0))
        if ((ref == 0) & (nv == 31)).any():
            j = int(np.nonzero((ref == 0) & (nv == 31))[0][0])
            assert len(a.track(int(ids[j]))["slots"]) == 32


# ---- 4: the 30-clone run with no track integer on the host -------------------------------------------------------------
def test_window30_run_with_candidates_and_counters_from_the_store():
    run = window30.Run()
    events = track_events.derive(run)
    z = run.z
    params = run.select_params()
    gyro, acc = nominal_ref.raw_samples(run)
    keys, updates, split_updates, prunes = [], 0, 0, 0
    with _engine(max_clones=31, max_track=31) as eng:
        eng.set_prior(z["P0"], z["gravity"], z["K"], run.sigma)
        eng.set_nominal(z["imu_R0"][0], z["imu_t0"][0], z["imu_v0"][0], z["gravity"], z["Qc"],
                        T_W_I=(z["T_W_I_R"], z["T_W_I_t"]), T_W_C=(z["T_W_C_R"], z["T_W_C_t"]))
        for kind, idx, o in nominal_ref.imu_groups(run):
            if kind == "imu":
                eng.propagate_imu(gyro[idx], acc[idx], z["imu_dt"][idx])
                continue
            if kind == AUGMENT:
                eng.augment_imu()
                keys.append(int(run.aug(idx)["key"]))
                continue
            assert kind in (PROCESS, PRUNE)
            c, ev = run.call(idx), events[idx]
            assert c["keys"].tolist() == keys and eng.n_clones == len(keys)
            if kind == PROCESS:
                # the frame's matches: the fixture's generator bypassed the tests, so nothing may fail them
                pool = ev["observe_pool"]
                res, fail = eng.tracks_frame(ev["observe_ids"], z["pool_uv"][pool].astype(np.float64),
                                             z["pool_score"][pool].astype(np.float64), z["K"], INF, INF)
                assert np.isin(res, (0, 4)).all() and (fail == -1).all(), idx
                ids = eng.load_tracks_where()
            else:
                assert len(ev["observe_ids"]) == 0
                views = eng.tracks_clone_views()
                want = np.zeros(len(keys), np.int32)
                for k, n in c["counts"].tolist():
                    want[keys.index(int(k))] = n
                assert np.array_equal(views, want), idx
                prunes += 1
                ids = eng.load_tracks_where(ev["rm"])
            assert np.array_equal(ids, c["ids"]), idx
            lost, tracked = eng.tracks_counters(ids)
            assert np.array_equal(lost, c["lost"]) and np.array_equal(tracked, c["tracked"]), idx
            eng.run_select(params, z["K"])
            sel = eng.selection()
            assert np.array_equal(sel.flags, c["flags"]), idx
            n_valid = int(sel.valid.sum())
            if 0 < n_valid < 0.15 * len(ids):
                eng.replan()
            if n_valid:
                eng.run()
                r = eng.result()
                assert r.status == c["status"] and r.n_rejected == c["n_rejected"], idx
                assert np.array_equal(r.accepted, c["accepted"]), idx
                if r.status == 0:
                    updates += 1
                    split_updates += int(eng.debug_split()["long_tracks"] > 0)
                    e = rel_err(r.dx, c["dx"])
                    assert e < TOL, (idx, e)
                assert eng.commit_inject() == r.status
            else:
                assert c["status"] == 1
            eng.tracks_remove(ev["remove"])
            if len(ev["rm"]):
                eng.remove_clones(ev["rm"])
                keys = [k for s, k in enumerate(keys) if s not in ev["rm"]]
                assert sorted(eng.tracks_dropped().tolist()) == ev["dropped"], idx
            assert eng.tracks_count() == (len(c["exit_ids"]), int(c["exit_nview"].sum())), idx
    assert split_updates >= 10 and prunes >= 8, (updates, split_updates, prunes)


# ---- 5: hand-built cases -------------------------------------------------------------------------------------------------
def _small(N, F, seed):
    from msckf_amd import synth
    p = synth.make_problem(N, F, N, seed=seed)
    return p, np.asarray(p.obs_uv, dtype=np.float64).reshape(F, N, 2)


def _start(eng, p):
    eng.set_prior(np.eye(15) * 0.01, p.gravity, p.K, p.sigma)


def _clone(eng, p, s):
    eng.augment(frame_cases.J15, p.cam_R[s], p.cam_t[s])


def _frame(eng, p, ids, uv, thr=(INF, INF)):
    return eng.tracks_frame(ids, uv, np.full(len(ids), 0.5), p.K, thr[0], thr[1])


def test_creation_order_survives_recycled_rows_and_candidates_follow_the_slots():
    from msckf_amd import synth
    p, uv = _small(4, 5, seed=21)
    with _engine(max_clones=5, max_features=5, max_track=5) as eng:
        _start(eng, p)
        _clone(eng, p, 0)
        res, _ = _frame(eng, p, [11, 3], uv[[0, 1], 0])
        assert res.tolist() == [4, 4]
        _clone(eng, p, 1)
        res, _ = _frame(eng, p, [7, 11, 20], uv[[2, 0, 3], 1])
        assert res.tolist() == [4, 0, 4]
        assert eng.load_tracks_where().tolist() == [11, 3, 7, 20]
        assert eng.load_tracks_where([1]).tolist() == [11, 7, 20] and eng.load_tracks_where([0]).tolist() == [11, 3]
        assert eng.tracks_clone_views().tolist() == [2, 3]
        eng.tracks_remove([3])                                       # its row goes back on the stack ...
        _clone(eng, p, 2)
        res, _ = _frame(eng, p, [5, 20], uv[[4, 3], 2])               # ... and 5 takes it: still the youngest track
        assert res.tolist() == [4, 0]
        assert eng.load_tracks_where().tolist() == [11, 7, 20, 5]
        assert eng.load_tracks_where([2, 0]).tolist() == [11, 20, 5]
        assert eng.tracks_counters([11, 7, 20, 5]) [0].tolist() == [1, 1, 0, 0]
        assert eng.tracks_counters([11, 7, 20, 5])[1].tolist() == [2, 1, 2, 1]
        assert eng.tracks_clone_views().tolist() == [1, 3, 2]
        eng.remove_clones([1])                                       # 7 had its only view there
        assert eng.tracks_dropped().tolist() == [7] and eng.tracks_clone_views().tolist() == [1, 2]
        assert eng.tracks_counters([11, 20, 5])[1].tolist() == [2, 2, 1]      # never decremented
        _clone(eng, p, 3)
        assert eng.tracks_clone_views().tolist() == [1, 2, 0]         # a clone without features
        # no candidate: as load_tracks([])
        assert eng.load_tracks_where([2]).size == 0
        eng.run_select(synth.SelectParams(min_frames_lost=1, min_frames_tracked=2, use_parallax=False, min_parallax_deg=0.0), p.K)
        eng.run()
        assert eng.result().status == 1


def test_counters_over_a_hole_and_a_failing_match():
    p, uv = _small(5, 3, seed=22)
    tight = (1e-9, 1e-9)
    with _engine(max_clones=5, max_features=4, max_track=5) as eng:
        _start(eng, p)
        _clone(eng, p, 0)
        _frame(eng, p, [1, 2, 3], uv[:, 0])
        _clone(eng, p, 1)
        _frame(eng, p, [1, 3], uv[[0, 2], 1])
        assert eng.tracks_counters([1, 2, 3])[0].tolist() == [0, 1, 0]
        _clone(eng, p, 2)
        _frame(eng, p, [1], uv[[0], 2])
        assert eng.tracks_counters([1, 2, 3])[0].tolist() == [0, 2, 1]
        _clone(eng, p, 3)
        res, _ = _frame(eng, p, [2, 1], uv[[1, 0], 3])               # listed again: back to 0
        assert res.tolist() == [0, 0]
        lost, tracked = eng.tracks_counters([1, 2, 3])
        assert lost.tolist() == [0, 0, 2] and tracked.tolist() == [4, 2, 2]
        assert eng.track(2)["slots"].tolist() == [0, 3]
        # a keypoint 200 px off under tight thresholds: nothing appended, lost_for + 1
        _clone(eng, p, 4)
        # (the score is signed: one of the two directions is the failing side of the first view's epipolar line)
        failed = 0
        for shift in (200.0, -200.0):
            before, count = eng.track(1), eng.tracks_count()
            lost0, tracked0 = (int(x[0]) for x in eng.tracks_counters([1]))
            res, fail = _frame(eng, p, [1], uv[[0], 4] + np.array([0.0, shift]), thr=(1e-6, 1e-6))
            if res[0] == 0:
                eng.remove_clones([4])                               # takes the appended view along
                _clone(eng, p, 4)
                continue
            failed += 1
            after = eng.track(1)
            assert res[0] == 1 and fail[0] >= 0
            assert all(np.array_equal(before[k], after[k]) for k in before) and eng.tracks_count() == count
            lost, tracked = eng.tracks_counters([1])
            assert lost[0] == lost0 + 1 and tracked[0] == tracked0     # (tracked_for is never decremented: 5 after a passing first try)
            break
        assert failed == 1


def test_the_resident_pose_is_what_is_tested_against():
    p, uv = _small(3, 1, seed=23)
    with _engine(max_clones=4, max_features=4, max_track=4) as eng:
        _start(eng, p)
        _clone(eng, p, 0)
        eng.tracks_observe([1, 2], uv[[0, 0], 0], [0.5, 0.5])        # two tracks with the same view: the same pair twice
        _clone(eng, p, 1)
        _clone(eng, p, 2)
        far = uv[[0], 2] + np.array([0.0, 150.0])
        # no epipolar score exceeds +inf and every homography score exceeds -1: only the homography branch can fail
        r1, f1 = eng.tracks_frame([1], far, [0.5], p.K, INF, -1.0)
        assert r1.tolist() == [0] and f1.tolist() == [-1]            # 30 cm from clone 0: the epipolar branch
        R = p.cam_R[:3].copy()
        t = p.cam_t[:3].copy()
        t[2] = t[0] + np.array([1e-3, 0.0, 0.0])
        eng.set_poses(R, t)                                          # the newest clone now sits 1 mm from the view's clone
        r2, f2 = eng.tracks_frame([2], far, [0.5], p.K, INF, -1.0)
        assert r2.tolist() == [2] and f2.tolist() == [0]
        assert eng.track(1)["slots"].tolist() == [0, 2] and eng.track(2)["slots"].tolist() == [0]


def test_error_codes_leave_store_and_counters_as_they_were():
    from msckf_amd import _ffi
    p, uv = _small(5, 4, seed=24)

    def code(*a, **k):
        with pytest.raises(_ffi.EngineError) as err:
            _frame(eng, p, *a, **k)
        return err.value.code

    def snap(ids):
        return eng.tracks_count(), [eng.track(i) for i in ids], [x.tolist() for x in eng.tracks_counters(ids)]

    def same(a, b):
        return a[0] == b[0] and a[2] == b[2] and all(np.array_equal(x[k], y[k]) for x, y in zip(a[1], b[1]) for k in x)

    with _engine(max_clones=5, max_features=4, max_track=4) as eng:
        _start(eng, p)
        assert code([1], uv[[0], 0]) == _ffi.ERR_STATE               # N = 0
        for s in range(3):
            _clone(eng, p, s)
            _frame(eng, p, [1, 2, 3], uv[:3, s])
        assert code([1], uv[[0], 2]) == _ffi.ERR_DUP_SLOT            # already seen in the newest clone
        _clone(eng, p, 3)
        _frame(eng, p, [1], uv[[0], 3])                               # 1 holds max_track views now
        _clone(eng, p, 4)
        eng.tracks_remove([3])
        eng.tracks_observe([3], uv[[2], 4], [0.5])
        s0 = snap([1, 2, 3])
        assert code([2, 2], uv[[1, 1], 4]) == _ffi.ERR_DUP_SLOT      # listed twice
        assert code([3], uv[[2], 4]) == _ffi.ERR_DUP_SLOT            # already seen in the newest clone
        assert code([-4], uv[[3], 4]) == _ffi.ERR_ARG
        assert code([8], np.array([[np.nan, 1.0]])) == _ffi.ERR_ARG
        assert code([8], np.array([[1.0, np.inf]])) == _ffi.ERR_ARG
        assert code([8, 9], uv[[3, 3], 4]) == _ffi.ERR_ARG           # four rows, three in use
        assert code([8, 1], uv[[3, 0], 4]) == _ffi.ERR_ARG           # 1 holds max_track views already
        bad_uv = np.array([uv[2, 4], [np.nan, 1.0]])                 # the first offending pair in list order decides the code
        assert code([3, 8], bad_uv) == _ffi.ERR_DUP_SLOT             # 3 is in the newest clone already; then a uv that is not finite
        assert code([8, 3], bad_uv[::-1]) == _ffi.ERR_ARG            # ... the two pairs swapped
        with pytest.raises(_ffi.EngineError) as err:
            eng.tracks_counters([1, 77])
        assert err.value.code == _ffi.ERR_ARG
        with pytest.raises(_ffi.EngineError) as err:
            eng.load_tracks_where([5])
        assert err.value.code == _ffi.ERR_ARG
        assert same(s0, snap([1, 2, 3]))
        res, _ = _frame(eng, p, [8], uv[[3], 4])                      # ... and the next valid call works
        assert res.tolist() == [4] and eng.load_tracks_where().tolist() == [1, 2, 3, 8]
        assert eng.tracks_counters([1, 2, 3, 8])[0].tolist() == [1, 2, 1, 0]
