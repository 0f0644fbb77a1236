"""The match's search window and distinctiveness margin on the device: `set_match_options`, `tracks_match(keypoints=)`,
`tracks_match_report`, and `tracks_match_frame` under the options (k_match_last_uv, k_match_argmax_opt, k_match_resolve_opt).

1  Every case of `match_options_ref.SHAPES` against the rule restated in NumPy, with the window alone, the margin alone and
   both: equal pairs and reason codes, |sim - ref| <= gamma_D |a| |b| (gamma_D = D u / (1 - D u), u = 2^-24, the bound of
   `test_gpu_tracks_match.py`).
2  The new kernels against the old on the reference's twelve frames: radius = +inf gives the ids, result codes, failing
   views and -- bit for bit -- similarities of an engine with the options off; with the options cleared again a run is
   bit-equal to a fresh engine's.
3  The window's centre follows an append and a k_track_drop compaction: intakes around a `remove_clones`, against the `Store`
   wrapper, frame by frame.
4  The aliasing case through `tracks_match_frame`: wrong pairs on the plain engine, none under the window, creations and
   counters as the model has them; a frame whose every pair the window eliminates is skipped with nothing changed.
5  Errors, each followed by a call that answers as a fresh engine does."""
import numpy as np
import pytest

import frame_cases
import match_options_ref as mo
import match_ref

pytestmark = pytest.mark.gpu

INF = float("inf")
K = np.array([[400.0, 0.0, 320.0], [0.0, 400.0, 240.0], [0.0, 0.0, 1.0]])
U = 2.0 ** -24


def _engine(**kw):
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=16, max_features=512, max_track=32)
    args.update(kw)
    return UpdateEngine(**args)


def _start(eng):
    eng.set_prior(np.eye(15) * 0.01, np.array([0.0, 0.0, -9.81]), K, 1.0)


def _clone(eng, s):
    eng.augment(frame_cases.J15, np.eye(3), np.array([0.2 * s, 0.0, 0.0]))


def _pose(s):
    return np.eye(3), np.array([0.2 * s, 0.0, 0.0])


def _frame(eng, uv, desc, first_new_id, min_cos=mo.MIN_COS):
    """A frame whose geometry never objects (thresholds +inf)."""
    return eng.tracks_match_frame(uv, desc, np.ones(len(desc)), K, first_new_id, min_cos, INF, INF)


def _seed_table(eng, c):
    """The case's table as tracks 1..T of one view each: the rows are the raw descriptors, the last keypoints uvA."""
    T = len(c["A"])
    _clone(eng, 0)
    ids, res, _, _ = _frame(eng, c["uvA"], c["A"], 1)
    assert ids.tolist() == list(range(1, T + 1)) and (res == 4).all()


@pytest.fixture(scope="module")
def cases():
    return {shape: mo.case(*shape) for shape in mo.SHAPES}


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mo.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pairs_and_reason_codes_equal_the_model(shape, cases):
    T, n, D = shape
    c = cases[shape]
    A, B = c["A"], c["B"]
    gamma = D * U / (1 - D * U)
    with _engine() as eng:
        _start(eng)
        _seed_table(eng, c)
        for name, (radius, margin) in mo.MODES.items():
            m = mo.guards(A, B, mo.MIN_COS, c["uvA"], c["uvB"], radius, margin)
            eng.set_match_options(radius, margin)
            runs = [eng.tracks_match(B, mo.MIN_COS, keypoints=c["uvB"]) + eng.tracks_match_report()]
            if name == "margin":                                        # no window: the call without keypoints applies the margin too
                runs.append(eng.tracks_match(B, mo.MIN_COS) + eng.tracks_match_report())
            want = np.full(n, -1)
            want[m.idx2] = m.idx1 + 1
            for got_ids, got_sim, rep_ids, why in runs:
                assert rep_ids.tolist() == list(range(1, T + 1)), name
                assert np.array_equal(why, m.why), (name, why.tolist(), m.why.tolist())
                assert np.array_equal(got_ids, want), name
                bound = gamma * np.linalg.norm(A[m.idx1].astype(np.float64), axis=1) * np.linalg.norm(B[m.idx2].astype(np.float64), axis=1)
                err = np.abs(got_sim[m.idx2].astype(np.float64) - m.S[m.idx1, m.idx2])
                if len(err):
                    print(name, "sim err / bound:", float((err / bound).max()))
                assert (err <= bound).all() and (got_sim[want < 0] == 0).all(), name
        assert eng.tracks_count() == (T, T)                             # the store is untouched


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def _fixture_run(eng, fx, frames, log):
    """The fixture's frames through `frame_from_extracted` with the reference's removals; per frame what the call returned,
    the match's report and the store's size."""
    z = fx.z
    min_cos, thr_e, thr_h = (float(x) for x in z["params"])
    keys, last_id = [], 0
    for f in frames:
        fr = fx.frame(f)
        eng.augment(frame_cases.J15, fr["R"], fr["t"])
        keys.append(int(fr["key"]))
        had = eng.tracks_count()[0]
        _, out = eng.frame_from_extracted(fr["kp"], fr["desc"], fr["score"], z["K"], last_id + 1, min_cosine_similarity=min_cos,
                                          epipolar_threshold=thr_e, homography_threshold=thr_h)
        assert (out is None) == bool(fr["skipped"]), f
        log.append((f, out, eng.tracks_match_report() if had else None, eng.tracks_count()))
        last_id = int(fr["last_id"])
        if len(fr["rm_tracks"]):
            eng.tracks_remove(fr["rm_tracks"])
        rm = [keys.index(int(c)) for c in fr["rm_keys"] if int(c) in keys]
        if rm and len(rm) < len(keys):
            eng.remove_clones(rm)
            keys = [c for s, c in enumerate(keys) if s not in rm]


def _same_logs(x, y, bitwise_sim_everywhere):
    assert len(x) == len(y)
    for (f, out_a, rep_a, cnt_a), (_, out_b, rep_b, cnt_b) in zip(x, y):
        assert cnt_a == cnt_b and (out_a is None) == (out_b is None), f
        if rep_a is not None:
            assert np.array_equal(rep_a[0], rep_b[0]) and np.array_equal(rep_a[1], rep_b[1]), (f, rep_a[1].tolist(), rep_b[1].tolist())
            assert set(rep_a[1].tolist()) <= {0, 2, 3}
        if out_a is None:
            continue
        for k in range(3):                                              # ids, result codes, failing views
            assert np.array_equal(out_a[k], out_b[k]), (f, k)
        paired = np.ones(len(out_a[1]), dtype=bool) if bitwise_sim_everywhere else out_a[1] != 4
        assert np.array_equal(out_a[3][paired].view(np.uint32), out_b[3][paired].view(np.uint32)), f


def test_an_infinite_window_runs_the_new_kernels_and_equals_the_old():
    fx = match_ref.Fixture()
    frames = range(fx.n_frames)
    new, old, again, fresh = [], [], [], []
    with _engine() as a, _engine() as b:
        _start(a)
        _start(b)
        a.set_match_options(INF, None)
        _fixture_run(a, fx, frames, new)
        _fixture_run(b, fx, frames, old)
        _same_logs(new, old, False)
        codes = np.concatenate([rep[1] for _, _, rep, _ in new if rep is not None])
        assert {0, 2, 3} == set(codes.tolist())
        # the options cleared: the plain kernels again, bit-equal to an engine that never had them
        a.set_match_options(None, None)
        _start(a)
        _fixture_run(a, fx, range(4), again)
        ids = fx.frame(3)["out_ids"].tolist()                            # (behind frame 3's removals)
        with _engine() as c:
            _start(c)
            _fixture_run(c, fx, range(4), fresh)
            _same_logs(again, fresh, True)
            assert a.tracks_count() == c.tracks_count() == (len(ids), int(fx.frame(3)["out_ptr"][-1])) and len(ids) > 0
            for i in ids:
                ta, tc = a.track(i), c.track(i)
                assert all(np.array_equal(ta[k], tc[k]) for k in ta), i
                for p, q in zip(a.track_descriptor(i), c.track_descriptor(i)):
                    assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), i


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _sequence():
    """Six tracks 100 px apart that move 15 px a frame under a window of 20 px: a keypoint is inside its track's window only
    if the centre is the track's LAST keypoint.  Frame 2 brings two strangers, whose tracks go with the clone."""
    rng = np.random.default_rng(31)
    D = 8
    base = np.array([mo._unit(rng.standard_normal(D)) for _ in range(6)])
    p0 = np.column_stack([100.0 + 100.0 * (np.arange(6) % 3), 100.0 + 100.0 * (np.arange(6) // 3)])
    step = np.array([15.0, 0.0])

    def seen(which, at):
        order = rng.permutation(len(which))
        d = base[which] * rng.uniform(0.95, 1.05, (len(which), 1)) + 0.02 * rng.standard_normal((len(which), D)) / np.sqrt(D)
        return at[which][order], d[order].astype(np.float32)

    every = np.arange(6)
    f0 = (p0, base.astype(np.float32))
    f1 = seen(every, p0 + step)
    kp, d = seen(every, p0 + 2 * step)                                   # 15 px from frame 1's keypoints, 30 from frame 0's
    strangers = np.array([mo._unit(rng.standard_normal(D)) for _ in range(2)], dtype=np.float32)
    f2 = (np.concatenate([kp, [[500.0, 50.0], [500.0, 400.0]]]), np.concatenate([d, strangers]))
    kp, d = seen(every[:5], p0)                                          # 15 px from frame 1's keypoints, 30 from frame 2's
    f3 = (np.concatenate([kp, [[560.0, 240.0]]]), np.concatenate([d, strangers[:1]]))
    return [f0, f1, f2, f3]


def test_the_window_centre_follows_appends_and_removed_clones():
    frames = _sequence()
    store = mo.Store(K, mo.MIN_COS, INF, INF, radius=mo.RADIUS, margin=mo.MARGIN)
    seen = []
    with _engine(max_features=20) as eng:
        _start(eng)
        eng.set_match_options(mo.RADIUS, mo.MARGIN)                      # before the first intake: the empty store takes the options' path too

        def intake(key, kp, d):
            _clone(eng, key)
            store.add_camera(key, *_pose(key))
            table, first_new_id = list(store.table_ids), store.last_id + 1
            want = store.intake(key, kp, d, np.ones(len(d)))
            got = _frame(eng, kp, d, first_new_id)
            assert (want is None) == (got is None), key
            if table:
                rep_ids, why = eng.tracks_match_report()
                assert rep_ids.tolist() == table and np.array_equal(why, store.last.why), (key, why.tolist(), store.last.why.tolist())
                seen.extend(why.tolist())
            if want is not None:
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), key
            ids = list(store.tracks)
            assert eng.tracks_count() == (len(ids), sum(len(t.uv) for t in store.tracks.values()))
            lost, tracked = eng.tracks_counters(ids)
            assert lost.tolist() == [store.tracks[i].lost for i in ids] and tracked.tolist() == [store.tracks[i].tracked for i in ids]
            return want

        assert (intake(0, *frames[0])[1] == 4).all()
        assert (intake(1, *frames[1])[1] == 0).all()                   # frame 0's keypoints are the centres
        out = intake(2, *frames[2])                                    # the appended keypoints are: frame 0's are 30 px away
        assert sorted(out[1].tolist()) == [0] * 6 + [4] * 2
        gone = store.remove_cameras([2])
        eng.remove_clones([2])
        assert sorted(eng.tracks_dropped().tolist()) == sorted(gone) and len(gone) == 2
        out = intake(3, *frames[3])                                    # ... and now frame 1's again, 30 px from frame 2's
        assert sorted(out[1].tolist()) == [0] * 5 + [4] and store.last.why.tolist().count(1) == 1
        assert len(store.tracks) <= 20 and {0, 1} <= set(seen)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_aliasing_through_the_frame_intake(cases):
    c = cases[(48, 48, 64)]
    T, n = len(c["A"]), len(c["B"])
    plain_model = match_ref.Store(K, mo.MIN_COS, INF, INF)
    window_model = mo.Store(K, mo.MIN_COS, INF, INF, radius=mo.RADIUS)
    with _engine() as plain, _engine() as window:
        window.set_match_options(mo.RADIUS, None)
        wrong = {}
        for name, eng, model in (("plain", plain, plain_model), ("window", window, window_model)):
            _start(eng)
            _seed_table(eng, c)
            _clone(eng, 1)
            for key in (0, 1):
                model.add_camera(key, *_pose(key))
            model.intake(0, c["uvA"], c["A"], np.ones(T))
            want_ids, want_res, pairs = model.intake(1, c["uvB"], c["B"], np.ones(n))
            ids, res, _, _ = _frame(eng, c["uvB"], c["B"], T + 1)
            assert np.array_equal(ids, want_ids) and np.array_equal(res, want_res), name
            went = np.nonzero(res == 0)[0]
            true, wrong[name] = mo.score(c, ids[went] - 1, went)
            assert true + wrong[name] == len(pairs)
            all_ids = list(model.tracks)
            assert eng.tracks_count() == (len(all_ids), T + n)
            lost, tracked = eng.tracks_counters(all_ids)
            assert lost.tolist() == [model.tracks[i].lost for i in all_ids], name
            assert tracked.tolist() == [model.tracks[i].tracked for i in all_ids], name
        print("wrong pairs: plain", wrong["plain"], "window", wrong["window"])
        assert wrong["plain"] >= 1 and wrong["window"] == 0
        # the same descriptors at keypoints no window reaches: every pair is eliminated, the frame is skipped as a whole
        away = c["uvB"] + [1000.0, 0.0]
        all_ids = list(window_model.tracks)
        before = (window.tracks_count(), [x.tolist() for x in window.tracks_counters(all_ids)], [window.track(i) for i in all_ids[:50]],
                  [window.track_descriptor(i) for i in all_ids[:50]])
        _clone(window, 2)
        _clone(plain, 2)
        window_model.add_camera(2, *_pose(2))
        assert window_model.intake(2, away, c["B"], np.ones(n)) is None
        assert _frame(window, away, c["B"], T + n + 1) is None
        rep_ids, why = window.tracks_match_report()
        assert rep_ids.tolist() == all_ids and (why == 1).all() and (window_model.last.why == 1).all()
        after = (window.tracks_count(), [x.tolist() for x in window.tracks_counters(all_ids)], [window.track(i) for i in all_ids[:50]],
                 [window.track_descriptor(i) for i in all_ids[:50]])
        assert before[:2] == after[:2]
        assert all(np.array_equal(p[k], q[k]) for p, q in zip(before[2], after[2]) for k in p)
        assert all(np.array_equal(p[k], q[k]) for p, q in zip(before[3], after[3]) for k in (0, 1))
        assert _frame(plain, away, c["B"], 4 * (T + n)) is not None      # (without the window the same frame pairs)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_options_and_the_engine_as_they_were(cases):
    from msckf_amd import _ffi
    c = cases[(15, 16, 8)]
    B, uvB = c["B"], c["uvB"]

    def code(fn, *a, **k):
        with pytest.raises(_ffi.EngineError) as err:
            fn(*a, **k)
        return err.value.code

    def answer(eng):
        ids, sim = eng.tracks_match(B, mo.MIN_COS, keypoints=uvB)
        rep_ids, why = eng.tracks_match_report()
        return ids.tolist(), sim.view(np.uint32).tolist(), rep_ids.tolist(), why.tolist()

    with _engine() as fresh:
        _start(fresh)
        _seed_table(fresh, c)
        fresh.set_match_options(mo.RADIUS, mo.MARGIN)
        want = answer(fresh)
    m = mo.match(c["A"], B, mo.MIN_COS, c["uvA"], uvB, mo.RADIUS, mo.MARGIN)
    assert want[3] == m.why.tolist() and {1, 4} <= set(want[3])          # an answer only both options give
    with _engine() as eng:
        _start(eng)
        _seed_table(eng, c)
        assert eng.tracks_match_report()[0].tolist() == []               # the first intake met an empty store: no match ran
        eng.set_match_options(mo.RADIUS, mo.MARGIN)
        for bad in ((-1.0, mo.MARGIN), (mo.RADIUS, -0.5), (float("nan"), mo.MARGIN), (mo.RADIUS, float("nan")), (-INF, None)):
            assert code(eng.set_match_options, *bad) == _ffi.ERR_ARG
            assert answer(eng) == want
        assert code(eng.tracks_match, B, mo.MIN_COS) == _ffi.ERR_STATE   # no keypoints, and a radius is on
        assert answer(eng) == want
        for v in (np.nan, np.inf):
            kp = uvB.copy()
            kp[3, 1] = v
            assert code(eng.tracks_match, B, mo.MIN_COS, keypoints=kp) == _ffi.ERR_ARG
            assert code(_frame, eng, kp, B, 100) == _ffi.ERR_ARG
            assert answer(eng) == want
        with pytest.raises(ValueError):
            eng.tracks_match(B, mo.MIN_COS, keypoints=uvB[:-1])
        assert eng.tracks_count() == (15, 15)
        # sticky: a reset and a new state leave the options on, and empty the report
        eng.tracks_reset()
        assert eng.tracks_match_report()[0].tolist() == []
        _start(eng)
        _seed_table(eng, c)
        assert code(eng.tracks_match, B, mo.MIN_COS) == _ffi.ERR_STATE
        assert answer(eng) == want
        eng.set_match_options(None, mo.MARGIN)                           # the radius off: the call without keypoints is legal again
        ids, _ = eng.tracks_match(B, mo.MIN_COS)
        mm = mo.match(c["A"], B, mo.MIN_COS, margin=mo.MARGIN)
        expect = np.full(len(B), -1)
        expect[mm.idx2] = mm.idx1 + 1
        assert np.array_equal(ids, expect) and eng.tracks_match_report()[1].tolist() == mm.why.tolist()
