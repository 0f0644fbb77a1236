"""Frame intake from descriptors on the resident track store: `tracks_match`, `tracks_match_frame`, `track_descriptor`.

1  `tracks_match` against the restatement (`match_ref.match`) on five (T, n, D) shapes, the last over recycled rows: equal
   pairs, and |sim - ref| <= gamma_D |a| |b| with gamma_D = D u / (1 - D u), u = 2^-24 (a k-ordered fp32 fma chain of D
   products, whatever the order: Higham, Accuracy and Stability, 3.1); the inputs are first held to the 1e-4 guards.
2  Ties: duplicated frame descriptors go to the lowest keypoint, duplicated table rows to the earliest-created track.
3  The reference's twelve frames (`golden/match/match_frames.npz`) through the store, every frame.
4  The store after `tracks_match_frame` is bit-equal to one fed the same ids through `tracks_frame`.
5  Every error code, each followed by an unchanged store."""
import numpy as np
import pytest

import frame_cases
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


def _pixels(rng, n):
    return np.column_stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)])


def _intake(eng, desc, first_new_id, rng, min_cos=0.8):
    """A frame whose geometry never objects (thresholds +inf)."""
    n = len(desc)
    return eng.tracks_match_frame(_pixels(rng, n), desc, np.ones(n), K, first_new_id, min_cos, INF, INF)


def _table(eng, ids, D):
    return np.array([eng.track_descriptor(i)[0] for i in ids], dtype=np.float32).reshape(len(ids), D)


def _frame_for(rng, A, n, D):
    """n descriptors: noisy copies of table rows where there are rows to copy, strangers otherwise."""
    B = rng.standard_normal((n, D)) / np.sqrt(D)
    src = rng.permutation(len(A))[:max(1, (2 * n) // 3)]
    B[:len(src)] = A[src] * rng.uniform(0.9, 1.1, (len(src), 1)) + 0.1 * rng.standard_normal((len(src), D)) / np.sqrt(D)
    return B[rng.permutation(n)].astype(np.float32)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 4, False), (15, 17, 10, False), (17, 15, 64, False), (33, 50, 64, False), (130, 40, 64, True)]
MIN_COS = 0.5


def _case(T, n, D, recycled):
    """The inputs of one shape, from the first seed whose table and frame pass the 1e-4 guards (decided here, on the CPU)."""
    for seed in range(200):
        rng = np.random.default_rng(1000 * T + seed)
        c = dict(uv=[_pixels(rng, 130), _pixels(rng, 41)])
        if not recycled:
            c["A0"] = (rng.standard_normal((T, D)) * rng.uniform(0.7, 1.3, (T, 1)) / np.sqrt(D)).astype(np.float32)
            c["A"], c["order"] = c["A0"], list(range(1, T + 1))
        else:
            # 120 tracks, 30 of them deleted, 40 created over the freed rows and ten new ones: creation order != row order
            c["A0"] = (rng.standard_normal((120, D)) / np.sqrt(D)).astype(np.float32)
            c["gone"] = np.sort(rng.permutation(120)[:30] + 1)
            keep = [i for i in range(1, 121) if i not in set(c["gone"].tolist())]
            new = (rng.standard_normal((41, D)) / np.sqrt(D)).astype(np.float32)
            new[7] = c["A0"][keep[3] - 1] * 4.0                         # one keypoint that matches, or the frame is skipped
            c["new"], c["hit"] = new, keep[3]
            A = np.concatenate([c["A0"][np.asarray(keep) - 1], np.delete(new, 7, axis=0)])
            A[3] = ((A[3].astype(np.float64) + new[7].astype(np.float64)) / 2.0).astype(np.float32)   # two views, scores 1
            c["A"], c["order"] = A, keep + list(range(121, 161))
        c["B"] = _frame_for(rng, c["A"], n, D)
        try:
            assert match_ref.guards(c["A"], c["B"], MIN_COS, need_pairs=False)["pairs"] >= max(1, min(T, n) // 4)
        except AssertionError:
            continue
        return c
    raise AssertionError("no seed met the guards")


@pytest.mark.parametrize("T,n,D,recycled", SHAPES)
def test_match_equals_the_restatement(T, n, D, recycled):
    c = _case(T, n, D, recycled)
    A, B, order = c["A"], c["B"], c["order"]
    assert len(A) == T and len(B) == n
    with _engine() as eng:
        _start(eng)
        _clone(eng, 0)
        m = len(c["A0"])
        ids, res, _, _ = eng.tracks_match_frame(c["uv"][0][:m], c["A0"], np.ones(m), K, 1, 0.8, INF, INF)
        assert ids.tolist() == list(range(1, m + 1)) and (res == 4).all()
        if recycled:
            eng.tracks_remove(c["gone"])
            _clone(eng, 1)
            ids2, res2, _, _ = eng.tracks_match_frame(c["uv"][1], c["new"], np.ones(41), K, 121, 0.9, INF, INF)
            assert int((res2 == 4).sum()) == 40 and res2[7] == 0 and ids2[7] == c["hit"]
            assert np.delete(ids2, 7).tolist() == list(range(121, 161))
            assert eng.track(121)["slots"].tolist() == [1] and eng.tracks_count()[0] == T
        assert np.array_equal(_table(eng, order, D).view(np.uint32), A.view(np.uint32))
        idx1, idx2, S = match_ref.match(A, B, MIN_COS)
        got_ids, got_sim = eng.tracks_match(B, MIN_COS)
        want = np.full(n, -1)
        want[idx2] = np.asarray(order)[idx1]
        assert len(idx1) >= min(T, n) // 4 and len(idx1) >= 1
        assert np.array_equal(got_ids, want)
        gamma = D * U / (1 - D * U)
        bound = gamma * np.linalg.norm(A[idx1].astype(np.float64), axis=1) * np.linalg.norm(B[idx2].astype(np.float64), axis=1)
        err = np.abs(got_sim[idx2].astype(np.float64) - S[idx1, idx2])
        print("sim err / bound:", float((err / bound).max()))
        assert (err <= bound).all() and (got_sim[want < 0] == 0).all()
        assert eng.tracks_count()[0] == T                               # the store is untouched
        assert np.array_equal(_table(eng, order, D).view(np.uint32), A.view(np.uint32))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def test_duplicated_frame_descriptors_go_to_the_lowest_keypoint():
    rng = np.random.default_rng(7)
    a, b, c = (np.eye(16, dtype=np.float32)[k] for k in range(3))
    with _engine(max_features=3) as eng:
        _start(eng)
        _clone(eng, 0)
        ids, _, _, _ = _intake(eng, np.array([a, b, c]), 1, rng)
        assert ids.tolist() == [1, 2, 3]
        frame = np.array([c * 0.5, a, b * 0.5, a, a])                  # a three times: keypoint 1 gets it
        got, sim = eng.tracks_match(frame, 0.25)
        assert got.tolist() == [3, 1, 2, -1, -1] and sim.tolist() == [0.5, 1.0, 0.5, 0.0, 0.0]


def test_duplicated_table_rows_go_to_the_earliest_created_track():
    rng = np.random.default_rng(8)
    a, b, c = (np.eye(16, dtype=np.float32)[k] for k in range(3))
    with _engine(max_features=3) as eng:
        _start(eng)
        _clone(eng, 0)
        _intake(eng, np.array([a, b, c]), 1, rng)
        eng.tracks_remove([1])                                         # row 0 is free again ...
        _clone(eng, 1)
        # ... and goes to track 4, created from c: at 2.9 only 3 b . b = 3 is a match (c . c = 1 fails the threshold)
        ids, res, _, _ = _intake(eng, np.array([3 * b, c]), 4, rng, min_cos=2.9)
        assert ids.tolist() == [2, 4] and res.tolist() == [0, 4]
        assert np.array_equal(eng.track_descriptor(3)[0], c) and np.array_equal(eng.track_descriptor(4)[0], c)
        got, sim = eng.tracks_match(np.array([c]), 0.5)
        assert got.tolist() == [3] and sim.tolist() == [1.0]           # 3 is older; 4 sits in the lower row


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _ulp_ok(got32, ref64):
    ref64 = np.asarray(ref64, dtype=np.float64)
    return bool(np.all(np.abs(np.asarray(got32, dtype=np.float64) - ref64) <= np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)))


def _check_store(eng, fx, fr, stage, keys, f):
    want = fx.tracks(fr, stage)
    ids = list(want)
    assert eng.tracks_count() == (len(ids), int(fr[stage + "_ptr"][-1])), (f, stage)
    if not ids:
        return
    lost, tracked = eng.tracks_counters(ids)
    assert lost.tolist() == [want[i][1] for i in ids] and tracked.tolist() == [want[i][2] for i in ids], (f, stage)
    ptr, tid = fr[stage + "_ptr"], fr[stage + "_table_ids"].tolist()
    for k, i in enumerate(ids):
        row, views = eng.track_descriptor(i)
        assert eng.track(i)["slots"].tolist() == [keys.index(c) for c in want[i][0]], (f, stage, i)
        assert np.array_equal(views.view(np.uint32), fr[stage + "_desc"][ptr[k]:ptr[k + 1]].view(np.uint32)), (f, stage, i)
        assert _ulp_ok(row, fr[stage + "_table"][tid.index(i)]), (f, stage, i)


def test_the_reference_frames_through_the_store():
    fx = match_ref.Fixture()
    z = fx.z
    min_cos, thr_e, thr_h = (float(x) for x in z["params"])
    keys, last_id, seen = [], 0, dict(skipped=0, pruned=0, raw=0)
    with _engine() as eng:
        _start(eng)
        for f in range(fx.n_frames):
            fr = fx.frame(f)
            eng.augment(frame_cases.J15, fr["R"], fr["t"])
            keys.append(int(fr["key"]))
            raw = eng.tracks_count()[0] == 0
            kept, out = eng.frame_from_extracted(fr["kp"], fr["desc"], fr["score"], z["K"], last_id + 1, min_cosine_similarity=min_cos,
                                                 epipolar_threshold=thr_e, homography_threshold=thr_h)
            assert len(kept) == len(fr["kp"])                           # the fixture's scores all pass the floor
            assert (out is None) == bool(fr["skipped"]), f
            if out is None:
                seen["skipped"] += 1                                    # ... and _check_store finds everything as it was
            else:
                ids, res, fail, sim = out
                assert np.array_equal(ids, fr["ids"]) and np.array_equal(res, fr["result"]), f
                assert np.array_equal(fail >= 0, (res == 1) | (res == 2))
                seen["raw"] += int(raw)
            last_id = int(fr["last_id"])
            _check_store(eng, fx, fr, "in", keys, f)
            if len(fr["rm_tracks"]):
                eng.tracks_remove(fr["rm_tracks"])
            rm = [keys.index(int(c)) for c in fr["rm_keys"] if int(c) in keys]
            if rm and len(rm) < len(keys):                              # (the reference drops every clone of an emptied store; the engine keeps them)
                eng.remove_clones(rm)
                keys = [c for s, c in enumerate(keys) if s not in rm]
                assert sorted(eng.tracks_dropped().tolist()) == fr["dropped"].tolist(), f
                seen["pruned"] += int(len(fr["dropped"]) > 0 and not len(fr["rm_tracks"]))
            _check_store(eng, fx, fr, "out", keys, f)                   # (behind a prune: compacted views, stale rows)
    assert seen == dict(skipped=1, pruned=1, raw=2), seen


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_the_store_is_the_one_tracks_frame_makes():
    fx = match_ref.Fixture()
    z = fx.z
    min_cos, thr_e, thr_h = (float(x) for x in z["params"])
    with _engine() as a, _engine() as b:
        for eng in (a, b):
            _start(eng)
        last_id = 0
        for f in range(4):
            fr = fx.frame(f)
            for eng in (a, b):
                eng.augment(frame_cases.J15, fr["R"], fr["t"])
            ids, res, fail, _ = a.tracks_match_frame(fr["kp"], fr["desc"], fr["score"], z["K"], last_id + 1, min_cos, thr_e, thr_h)
            res_b, fail_b = b.tracks_frame(ids, fr["kp"], fr["score"], z["K"], thr_e, thr_h)
            assert np.array_equal(res, res_b) and np.array_equal(fail, fail_b)
            last_id = int(fr["last_id"])
        assert {0, 1, 4} <= set(res.tolist())
        all_ids = fx.frame(3)["in_ids"].tolist()
        assert a.tracks_count() == b.tracks_count() == (len(all_ids), int(fx.frame(3)["in_ptr"][-1]))
        for x, y in zip(a.tracks_counters(all_ids), b.tracks_counters(all_ids)):
            assert np.array_equal(x, y)
        for i in all_ids:
            ta, tb = a.track(i), b.track(i)
            assert all(np.array_equal(ta[k], tb[k]) for k in ta), i
        assert a.load_tracks_where().tolist() == b.load_tracks_where().tolist() == all_ids


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_error_codes_leave_the_store_as_it_was():
    from msckf_amd import _ffi
    rng = np.random.default_rng(9)
    D = 8
    eye = np.eye(D, dtype=np.float32)

    def code(fn, *a, **k):
        with pytest.raises(_ffi.EngineError) as err:
            fn(*a, **k)
        return err.value.code

    def snap(ids):
        return (eng.tracks_count(), [x.tolist() for x in eng.tracks_counters(ids)], [eng.track(i) for i in ids],
                [eng.track_descriptor(i) for i in ids])

    def same(x, y):
        return (x[:2] == y[:2] and all(np.array_equal(p[k], q[k]) for p, q in zip(x[2], y[2]) for k in p)
                and all(np.array_equal(p[k], q[k]) for p, q in zip(x[3], y[3]) for k in (0, 1)))

    with _engine(max_features=4) as eng:
        _start(eng)
        assert code(eng.tracks_match, eye[:1], 0.5) == _ffi.ERR_STATE                       # N = 0
        assert code(_intake, eng, eye[:1], 1, rng) == _ffi.ERR_STATE
        _clone(eng, 0)
        ids, _, _, _ = _intake(eng, eye[:3], 1, rng)
        _clone(eng, 1)
        s0 = snap([1, 2, 3])
        bad = eye[:2].copy()
        bad[1, 3] = np.nan
        for fn in (lambda d, **k: eng.tracks_match(d, 0.5), lambda d, first=4: _intake(eng, d, first, rng)):
            assert code(fn, np.zeros((1, 65), np.float32)) == _ffi.ERR_ARG                  # D outside 1..64
            assert code(fn, np.zeros((1, 0), np.float32)) == _ffi.ERR_ARG
            assert code(fn, np.eye(4, dtype=np.float32)[:1]) == _ffi.ERR_ARG                # not the store's D
            assert code(fn, bad) == _ffi.ERR_ARG                                            # a non-finite descriptor
            bad[1, 3] = np.inf
        assert code(_intake, eng, eye[:2], -1, rng) == _ffi.ERR_ARG                         # first_new_id
        assert code(_intake, eng, eye[[0, 5]], 2, rng) == _ffi.ERR_ARG                      # ... collides with track 2
        assert code(_intake, eng, eye[[0, 5, 6]], 4, rng) == _ffi.ERR_ARG                   # two creations, one free row
        assert code(lambda: eng.tracks_match_frame(np.array([[np.nan, 1.0]]), eye[:1], [1.0], K, 4, 0.5, INF, INF)) == _ffi.ERR_ARG
        assert code(eng.track_descriptor, 77) == _ffi.ERR_ARG
        assert same(s0, snap([1, 2, 3]))
        assert _intake(eng, eye[5:6], 4, rng) is None and same(s0, snap([1, 2, 3]))         # no pair: skipped, nothing changed
        assert eng.tracks_match_frame(np.zeros((0, 2)), np.zeros((0, D), np.float32), [], K, 4) is None
        # a track that tracks_observe made has a view without a descriptor
        eng.tracks_observe([9], [[100.0, 100.0]], [0.5])
        s1 = snap([1, 2, 3])
        assert code(eng.tracks_match, eye[:1], 0.5) == _ffi.ERR_STATE
        assert code(_intake, eng, eye[:1], 10, rng) == _ffi.ERR_STATE
        assert code(eng.track_descriptor, 9) == _ffi.ERR_STATE
        assert same(s1, snap([1, 2, 3])) and eng.tracks_count() == (4, 4)
        eng.tracks_remove([9])
        ids, res, _, _ = _intake(eng, eye[[1, 6]], 10, rng)                                 # ... and the next valid call works
        assert ids.tolist() == [2, 10] and res.tolist() == [0, 4]
