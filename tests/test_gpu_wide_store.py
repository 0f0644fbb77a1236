"""The track store on a wide-track context: `UpdateEngine(max_track=64, wide_store=True)` (`MSCKF_FLAG_WIDE_STORE`), rows of up
to 64 views, the per-row kernels `k_track_emit<64>`, `k_track_drop<64>`, `k_track_frame<64>` with a wavefront per row.

1  A batch asked for by track id equals, bit for bit, the same arrays sent through `set_features` + `set_tracks` on a
   wide-track engine created WITHOUT the flag (the path tests/test_gpu_wide_tracks.py holds to the oracle): tracks of 31, 32,
   33, 48, 63 and 64 views among 1, 2 and 10, one that skips clones, one on slots 32..63 only; and it holds
   tests/test_gpu_wide_tracks.py's tolerances against `oracle.update` (dx, P+ 1e-8 relative; gamma rtol 1e-8, atol 1e-12; mask
   and rejected count equal; P+ bit-symmetric).  The stored directions against NumPy within 8 eps max|d|, m within 4 eps.
2  A subset in permuted order follows the given order; wide and narrow rows share a workgroup.
3  `remove_clones` on a 64-view row: views, slots, count, descriptors, the anchor; a window of 100 clones.
4  `tracks_frame` on rows of 1, 31, 32, 33 and 63 views against `oracle.associate` and `msckf_run_associate`; the full row.
5  `tracks_match_frame` on rows of 33 to 40 views, plain and with the window and the margin, against the restatements.
6  A short run with the nominal state resident: a 40-clone window, 45 frames, 12 tracks.
7  Without the flag nothing moved: `max_track` 30 and 32.
8  Error paths leave the store as it was; `tracks_reset` and `set_state` empty it.

The cases, and what the CPU file (tests/test_wide_store.py) shows about them, are in tests/wide_store_cases.py.  Every figure
is printed before it is asserted.  No test provokes a fault: every refusal is an argument check on the host."""
import numpy as np
import pytest

import wide_cases
import wide_store_cases as ws
from conftest import rel_err
from msckf_amd import _ffi, synth
from track_mirror_model import Model

pytestmark = pytest.mark.gpu

TOL = 1e-8
GAMMA_TOL = dict(rtol=1e-8, atol=1e-12)
EPS = ws.F64EPS
U32 = 2.0 ** -24
INF = ws.INF


def _params(refine_iters=0):
    return synth.SelectParams(**ws.PARAMS, refine_iters=refine_iters)


def _code(fn, *a, **k):
    with pytest.raises(_ffi.EngineError) as err:
        fn(*a, **k)
    return err.value.code


def _snapshot(eng, ids):
    return eng.tracks_count(), [eng.track(i) for i in ids], [x.tolist() for x in eng.tracks_counters(ids)]


def _same_snapshot(a, b):
    return a[0] == b[0] and a[2] == b[2] and all(np.array_equal(x[k], y[k]) for x, y in zip(a[1], b[1]) for k in x)


def _through_the_store(eng, ids, lost, tracked, params, K):
    eng.load_tracks(ids, lost, tracked)
    eng.run_select(params, K)
    sel = eng.selection()
    res, gam = None, None
    if int(sel.valid.sum()):
        eng.run()
        res = eng.result()
        gam = eng.debug_gate()[0]
    return sel, res, gam


def _hold_to_the_oracle(b, P, cam_R, cam_t, gravity, K, sigma, sel, res, gam, what):
    """`oracle.update` on the batch's valid tracks, fed the device's refreshed points, at tests/test_gpu_wide_tracks.py's tolerances."""
    prob = ws.problem_of(b, P, cam_R, cam_t, gravity, K, sigma)
    valid, out = ws.chained_reference(prob, sel.flags, sel.idp_m, sel.idp_rho)
    m = wide_cases.margin(out)
    e_dx, e_P = rel_err(res.dx, out["dx"]), rel_err(res.P_new, out["P_new"])
    e_g = float(np.max(np.abs(gam[valid] - out["gamma"]) / np.maximum(np.abs(out["gamma"]), 1e-300)))
    print(f"{what}: {len(valid)} valid, gate margin {m:.4f}, dx {e_dx:.2e} P+ {e_P:.2e} gamma {e_g:.2e} "
          f"accepted {int(res.accepted.sum())} rejected {res.n_rejected}", flush=True)
    assert m >= wide_cases.MIN_MARGIN, what
    assert res.status == out["status"] and res.n_rejected == out["n_rejected"], what
    assert np.array_equal(res.accepted[valid], out["accepted"]) and not np.delete(res.accepted, valid).any(), what
    assert e_dx < TOL and e_P < TOL, (what, e_dx, e_P)
    np.testing.assert_allclose(gam[valid], out["gamma"], **GAMMA_TOL)
    assert np.array_equal(res.P_new, res.P_new.T), what
    return out


# ---- 1: store batch = host batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine_iters", [0, 4])
@pytest.mark.parametrize("name", sorted(ws.UPDATE_CASES))
def test_store_batch_equals_the_host_batch_bit_for_bit(name, refine_iters):
    c = ws.update_case(name)
    p, uv, ids, views, lost, tracked, host = (c[k] for k in ("p", "uv", "ids", "views", "lost", "tracked", "host"))
    params = _params(refine_iters)
    with ws.wide_engine(max_clones=p.N) as eng, ws.door_engine(max_clones=p.N) as eng_b:
        ws.grow(eng, p, uv, views, ids)
        eng.import_covariance(p.P)
        assert eng.tracks_count() == (len(ids), sum(map(len, views)))
        tr, b = ws.store_batch(eng, ids)
        # the rows against NumPy
        for k in ("view_ptr", "obs_slot", "obs_uv", "line_base", "line_conf", "idp_base", "idp_rho"):
            assert np.array_equal(b[k], host[k]), (name, k)
        e_dir = float(np.abs(b["line_dir"] - host["line_dir"]).max() / (EPS * np.abs(host["line_dir"]).max()))
        e_m = float(np.abs(b["idp_m"] - host["idp_m"]).max() / EPS)
        print(f"{name}: stored directions {e_dir:.2f} eps max|d| (bound 8), m {e_m:.2f} eps (bound 4)", flush=True)
        assert e_dir <= 8 and e_m <= 4
        assert [t["anchor_slot"] for t in tr] == [v[0] for v in views]
        # through both doors
        sel_b, res_b = ws.host_door(eng_b, b, p.P, p.cam_R, p.cam_t, p.gravity, p.K, p.sigma, lost, tracked, params)
        gam_b = eng_b.debug_gate()[0]
        sel, res, gam = _through_the_store(eng, ids, lost, tracked, params, p.K)
        ws.same_through_both_doors(sel, res, sel_b, res_b, name)
        valid = np.nonzero(sel.valid)[0]
        assert res is not None and np.array_equal(gam[valid], gam_b[valid])
        assert eng.debug_split() == eng_b.debug_split() and eng.debug_split()["band_plan"] == 0      # no split: the merge tree
        assert res.stats["stacked_rows"] == res_b.stats["stacked_rows"] and res.stats["n_leaves"] == res_b.stats["n_leaves"]
        if refine_iters:
            print(f"{name}: refine_iters {refine_iters}: refined points kept on {int(((sel.flags & 8) > 0).sum())} tracks", flush=True)
        else:
            assert np.array_equal(sel.flags & 7, c["sel"]["flags"] & 7)
            _hold_to_the_oracle(b, p.P, p.cam_R, p.cam_t, p.gravity, p.K, p.sigma, sel, res, gam, name)
        # the refreshed points went back to the rows (k_track_writeback)
        assert (sel.flags & 4).any()
        for j, i in enumerate(ids):
            t = eng.track(i)
            if sel.flags[j] & 4:
                assert np.array_equal(t["idp_m"], sel.idp_m[j]) and t["idp_rho"] == sel.idp_rho[j], (name, i)
            else:
                assert np.array_equal(t["idp_m"], tr[j]["idp_m"]) and t["idp_rho"] == 0.1, (name, i)


# ---- 2: emit order -----------------------------------------------------------------------------------------------------------
def test_a_subset_in_permuted_order_follows_the_given_order():
    """Five of w48's tracks, wide and narrow alternating: with a wavefront per row, four rows share a workgroup and the fifth
    starts the next."""
    c = ws.update_case("w48")
    p, uv, ids, views = c["p"], c["uv"], c["ids"], c["views"]
    nv = dict(zip(ids, map(len, views)))
    params = _params()
    out = {}
    with ws.wide_engine(max_clones=p.N) as eng, ws.door_engine(max_clones=p.N) as eng_b:
        ws.grow(eng, p, uv, views, ids)
        eng.import_covariance(p.P)
        for order in ([8, 5, 27, 41, 33], [33, 41, 27, 5, 8]):
            assert [nv[i] for i in order] in ([48, 2, 33, 1, 32], [32, 1, 33, 2, 48])
            lost = np.array([0 if i == 41 else 1 for i in order], np.int32)      # 41 has one view and is not lost: not valid
            tracked = np.array([nv[i] for i in order], np.int32)
            _, b = ws.store_batch(eng, order)
            assert b["view_ptr"].tolist() == np.concatenate([[0], np.cumsum(tracked)]).tolist()
            door = ws.host_door(eng_b, b, p.P, p.cam_R, p.cam_t, p.gravity, p.K, p.sigma, lost, tracked, params)
            sel, res, _ = _through_the_store(eng, order, lost, tracked, params, p.K)
            ws.same_through_both_doors(sel, res, door[0], door[1], order)
            assert [bool(v) for v in sel.valid] == [i != 41 for i in order] and res.accepted[order.index(41)] == 0
            out[tuple(order)] = {i: (int(sel.flags[k]), int(res.accepted[k])) for k, i in enumerate(order)}
            # (no commit: the second order starts from the same prior, and the selection refreshes the same points again)
    a, b = out.values()
    assert a == b


# ---- 3, 5: stores fed by descriptors ----------------------------------------------------------------------------------------
def _ulp_ok(got32, ref64):
    ref64 = np.asarray(ref64, dtype=np.float64)
    return bool(np.all(np.abs(np.asarray(got32, dtype=np.float64) - ref64) <= np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)))


def _walk(eng, p, frames, log, report=False):
    """The frames through `tracks_match_frame`, one clone each, against the restatement's log: ids, codes, and (report) the
    match table's reason codes and the similarities."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((15, 15))
    eng.set_prior(A @ A.T / 15 + np.eye(15) * 0.1, p.gravity, p.K, p.sigma)
    last_id, worst = 0, 0.0
    for s, (kp, d, sc, _) in enumerate(frames):
        eng.augment(ws.J15, p.cam_R[s], p.cam_t[s])
        if len(kp) == 0:
            assert log[s] is None
            continue                                                 # (`MSCKF.py:286`: the caller does not call)
        out = eng.tracks_match_frame(kp, d, sc, p.K, last_id + 1, ws.MIN_COS, INF, INF)
        assert (out is None) == (log[s] is None), s
        if out is None:
            continue
        ids, res, fail, sim = out
        want_ids, want_res, why, table_ids, want_sim = log[s]
        assert np.array_equal(ids, want_ids) and np.array_equal(res, want_res) and (fail == -1).all(), s
        last_id = max(last_id, int(ids.max()))
        if report and why is not None:
            rep_ids, rep_why = eng.tracks_match_report()
            assert rep_ids.tolist() == table_ids and np.array_equal(rep_why, why), s
            gamma = ws.DESC_D * U32 / (1 - ws.DESC_D * U32)
            hit = want_sim != 0
            err = np.abs(sim.astype(np.float64) - want_sim)
            assert np.array_equal(sim != 0, hit), s
            if hit.any():                                            # |a| = |b| = 1 up to fp32 rounding: bound gamma_D |a| |b|
                worst = max(worst, float(err[hit].max() / (gamma * 1.001)))
    return worst


def _check_rows(eng, st, slot_of):
    """Every track of the restatement as the store holds it: slots, keypoints, scores, per-view descriptors, counters."""
    assert eng.tracks_count() == (len(st.tracks), sum(len(t.uv) for t in st.tracks.values()))
    for i, tr in st.tracks.items():
        t = eng.track(i)
        row, views = eng.track_descriptor(i)
        assert t["slots"].tolist() == [slot_of[k] for k in tr.keys], i
        assert np.array_equal(t["uv"], np.array(tr.uv).reshape(-1, 2)) and np.array_equal(t["conf"], np.array(tr.score)), i
        assert np.array_equal(views.view(np.uint32), np.array(tr.desc, dtype=np.float32).view(np.uint32)), i
        if i in st.table_ids:
            assert _ulp_ok(row, st.table[st.table_ids.index(i)]), i
    ids = list(st.tracks)
    lost, tracked = eng.tracks_counters(ids)
    assert lost.tolist() == [st.tracks[i].lost for i in ids] and tracked.tolist() == [st.tracks[i].tracked for i in ids]


def _drop_and_check(eng, eng_b, p, c, rm, what):
    N = p.N
    st, log = ws.walk_model(p, c["frames"])
    _walk(eng, p, c["frames"], log)
    _check_rows(eng, st, {s: s for s in range(N)})
    ids = list(st.tracks)
    wide = next(i for i in ids if len(st.tracks[i].uv) == 64)
    before = {i: (eng.track(i), eng.track_descriptor(i)) for i in ids}
    cam_t = p.cam_t.copy()
    eng.remove_clones(rm)
    gone = st.remove_cameras(set(rm))
    keep = [s for s in range(N) if s not in rm]
    remap = {s: k for k, s in enumerate(keep)}
    print(f"{what}: clones {rm[:4]}{'...' if len(rm) > 4 else ''} go; tracks dropped {sorted(gone)}; the 64-view row keeps "
          f"{len(st.tracks[wide].uv) if wide in st.tracks else 0} views", flush=True)
    assert sorted(eng.tracks_dropped().tolist()) == sorted(gone)
    _check_rows(eng, st, remap)                                      # (slots renumbered, count, descriptors, the stale rows)
    for i in st.tracks:
        t, (b, (brow, bviews)) = eng.track(i), before[i]
        sel = [k for k, s in enumerate(b["slots"].tolist()) if s not in rm]
        for k in ("uv", "dir", "conf"):
            assert np.array_equal(t[k], b[k][sel]), (what, i, k)
        row, views = eng.track_descriptor(i)
        assert np.array_equal(views.view(np.uint32), bviews[sel].view(np.uint32)), (what, i)
        assert np.array_equal(row.view(np.uint32), brow.view(np.uint32)), (what, i)              # a snapshot: stale until the next intake
        assert np.array_equal(t["line_base"], cam_t[keep][t["slots"]])
        first = int(b["slots"][0])
        if first in rm:                                              # the anchor went: frozen at that clone's position
            assert t["anchor_slot"] == -1 and np.array_equal(t["idp_base"], cam_t[first]), (what, i)
        else:
            assert t["anchor_slot"] == remap[first] and np.array_equal(t["idp_base"], cam_t[first]), (what, i)
        assert np.array_equal(t["idp_m"], b["idp_m"]) and t["idp_rho"] == b["idp_rho"]
    # a following batch through both doors
    live = list(st.tracks)
    if live:
        n = len(keep)
        P = synth.random_spd_covariance(15 + 6 * n, np.random.default_rng(17))
        eng.import_covariance(P)
        lost, tracked = np.ones(len(live), np.int32), np.array([len(st.tracks[i].uv) for i in live], np.int32)
        _, b = ws.store_batch(eng, live)
        door = ws.host_door(eng_b, b, P, p.cam_R[keep], cam_t[keep], p.gravity, p.K, p.sigma, lost, tracked, _params())
        sel, res, _ = _through_the_store(eng, live, lost, tracked, _params(), p.K)
        ws.same_through_both_doors(sel, res, door[0], door[1], what)
        assert sel.valid.any() and res is not None
        # (the selection refreshed points in the rows; the model keeps none, and the next frame reads none)
    # the next frame: every live track is seen again, the rows are recomputed from the compacted views
    if live:
        rng = np.random.default_rng(23)
        kp = np.array([st.tracks[i].uv[-1] for i in live]) + rng.uniform(-2, 2, (len(live), 2))
        d = np.array([st.tracks[i].desc[-1] for i in live], dtype=np.float32)
        sc = rng.uniform(0.3, 1.0, len(live))
        R, t = p.cam_R[keep[-1]], cam_t[keep[-1]] + np.array([0.15, 0.0, 0.0])
        eng.augment(ws.J15, R, t)
        st.add_camera(N, R, t)
        want = st.intake(N, kp, d, sc)
        out = eng.tracks_match_frame(kp, d, sc, p.K, st.last_id + 1, ws.MIN_COS, INF, INF)
        assert want is not None and out is not None
        assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1]) and (out[1] == 0).all()
        remap[N] = len(keep)
        _check_rows(eng, st, remap)


@pytest.mark.parametrize("name", sorted(ws.DROP_SETS))
def test_remove_clones_on_a_row_of_64_views(name):
    c = ws.drop_case()
    with ws.wide_engine(max_clones=65) as eng, ws.door_engine(max_clones=65) as eng_b:
        _drop_and_check(eng, eng_b, c["p"], c, ws.DROP_SETS[name], name)


def test_remove_clones_on_a_window_of_100_clones():
    c = ws.drop100_case()
    with ws.wide_engine(max_clones=101) as eng, ws.door_engine(max_clones=101) as eng_b:
        _drop_and_check(eng, eng_b, c["p"], c, ws.DROP100_SET, "100 clones")


@pytest.mark.parametrize("mode", sorted(ws.MATCH_MODES))
def test_descriptor_intake_on_rows_of_33_to_40_views(mode):
    c = ws.match_case()
    p = c["p"]
    radius, margin = ws.MATCH_MODES[mode]
    st, log = ws.walk_model(p, c["frames"], radius, margin)
    with ws.wide_engine(max_clones=p.N) as eng:
        if radius or margin:
            eng.set_match_options(radius, margin)
        worst = _walk(eng, p, c["frames"], log, report=True)
        print(f"{mode}: worst similarity error / (gamma_D |a| |b|) {worst:.3f}", flush=True)
        assert worst <= 1.0
        _check_rows(eng, st, {s: s for s in range(p.N)})
        assert sorted(len(eng.track(i)["slots"]) for i in st.tracks)[-8:] == list(range(33, 41))


# ---- 4: frame intake ----------------------------------------------------------------------------------------------------------
def test_frame_intake_on_rows_of_1_to_63_views():
    c = ws.frame_case()
    p, uv, ids, views, new_uv, score = (c[k] for k in ("p", "uv", "ids", "views", "new_uv", "score"))
    n = len(ids)
    rng = np.random.default_rng(5)
    order = rng.permutation(n + 1)                                   # the fresh pair rides among the others
    all_ids = np.array(ids + [ws.FRAME_FRESH])[order]
    all_uv = np.concatenate([new_uv, [[123.0, 234.0]]])[order]
    all_score = score[order]
    back = np.argsort(order)
    with ws.wide_engine(max_clones=66) as a, ws.door_engine(max_clones=66) as b, ws.wide_engine(max_clones=66) as o:
        for eng in (a, o):
            ws.grow(eng, p, uv, views, ids)
            eng.augment(ws.J15, c["R_new"], c["t_new"])
        res, fail = a.tracks_frame(all_ids, all_uv, all_score, p.K, ws.THR_E, ws.THR_H)
        res_t, fail_t = res[back][:n], fail[back][:n]
        print("tracks_frame: result", res_t.tolist(), "fail_view", fail_t.tolist(), flush=True)
        assert res[back][n] == 4 and fail[back][n] == -1
        assert np.array_equal(res_t, c["res"]) and np.array_equal(fail_t, c["fail"])
        b.load(c["prob"])
        res_b, fail_b = b.associate(new_uv, c["R_new"], c["t_new"], p.K, ws.THR_E, ws.THR_H)
        assert np.array_equal(res_t, res_b) and np.array_equal(fail_t, fail_b)
        # the store is the one tracks_observe of the passing and the fresh pairs makes
        keep = (res == 0) | (res == 4)
        o.tracks_observe(all_ids[keep], all_uv[keep], all_score[keep])
        assert a.tracks_count() == o.tracks_count() == (n + 1, sum(map(len, views)) + int(keep.sum()))
        for i in all_ids.tolist():
            ta, to = a.track(i), o.track(i)
            assert all(np.array_equal(ta[k], to[k]) for k in ta), i
        assert a.track(ws.FRAME_FRESH)["slots"].tolist() == [63] and len(a.track(ws.FRAME_FULL)["slots"]) == 64
        # the counters against the mirror's model
        m = Model()
        m.size(16, 64)
        for s in range(p.N):
            m.intake([ids[j] for j in range(n) if s in views[j]], [1] * n, [0] * n, s, False, False)
        assert m.intake(all_ids.tolist(), [1] * (n + 1), res.tolist(), 63, True, False)[0] == 0
        lost, tracked = a.tracks_counters(all_ids)
        assert lost.tolist() == [m.live[i]["lost"] for i in all_ids.tolist()]
        assert tracked.tolist() == [m.live[i]["tracked"] for i in all_ids.tolist()]
        assert a.load_tracks_where().tolist() == m.ids_created_order()
        # a pair on the full row: the mirror's refusal, and the store is as it was
        a.augment(ws.J15, p.cam_R[-1], p.cam_t[-1] + np.array([0.15, 0.0, 0.0]))
        snap = _snapshot(a, all_ids.tolist())
        assert _code(a.tracks_frame, [ws.FRAME_FULL], new_uv[:1], [0.5], p.K, INF, INF) == _ffi.ERR_ARG
        assert _code(a.tracks_frame, [ids[1], ws.FRAME_FULL], new_uv[:2], [0.5, 0.5], p.K, INF, INF) == _ffi.ERR_ARG
        assert _code(a.tracks_observe, [ws.FRAME_FULL], new_uv[:1], [0.5]) == _ffi.ERR_ARG
        assert _same_snapshot(snap, _snapshot(a, all_ids.tolist()))
        r2, f2 = a.tracks_frame([ids[1]], new_uv[1:2], [0.5], p.K, INF, INF)          # ... and the store still works
        assert r2.tolist() == [0] and f2.tolist() == [-1] and a.track(ids[1])["slots"][-1] == 64


# ---- 6: a short resident run -----------------------------------------------------------------------------------------------------
def test_a_short_run_with_the_nominal_state_resident():
    K, g = synth.K_DEFAULT.copy(), synth.GRAVITY_DEFAULT.copy()
    params = _params()
    updates, wide_updates, worst = 0, 0, dict(dx=0.0, P=0.0)
    RUN_SIGMA, RUN_PRUNE = ws.RUN_SIGMA, ws.RUN_PRUNE
    with ws.wide_engine(max_clones=42) as eng, ws.door_engine(max_clones=42) as eng_b:
        for f, nom, seen, px, score in ws.run_frames(eng):
            res, fail = eng.tracks_frame(seen, px, score, K, INF, INF)
            assert np.isin(res, (0, 4)).all() and (fail == -1).all(), f
            prune = f == ws.RUN_PRUNE_AT
            ids = eng.load_tracks_where(RUN_PRUNE if prune else None)
            lost, tracked = eng.tracks_counters(ids)
            if not (lost > 0).any():
                if prune:
                    eng.remove_clones(RUN_PRUNE)
                continue
            # the same call through the host door, on the state as it stands on the device
            P = eng.covariance()
            _, b = ws.store_batch(eng, ids)
            door = ws.host_door(eng_b, b, P, nom["cam_R"], nom["cam_t"], g, K, RUN_SIGMA, lost, tracked, params)
            gam_b = eng_b.debug_gate()[0]
            eng.run_select(params, K)
            sel = eng.selection()
            assert sel.valid.any() and np.array_equal(sel.valid, lost > 0), f
            eng.run()
            r = eng.result()
            gam = eng.debug_gate()[0]
            ws.same_through_both_doors(sel, r, door[0], door[1], f)
            nv = np.diff(b["view_ptr"])
            out = _hold_to_the_oracle(b, P, nom["cam_R"], nom["cam_t"], g, K, RUN_SIGMA, sel, r, gam, f"frame {f}, views {nv[sel.valid].tolist()}")
            assert np.array_equal(gam[sel.valid], gam_b[sel.valid])
            worst["dx"], worst["P"] = max(worst["dx"], rel_err(r.dx, out["dx"])), max(worst["P"], rel_err(r.P_new, out["P_new"]))
            updates += 1
            wide_updates += int((nv[sel.valid] > 32).any())
            assert eng.commit_inject() == r.status
            eng.tracks_remove(ids[(sel.flags & _ffi.SEL_LOST) > 0])
            if prune:
                n0 = eng.tracks_count()
                eng.remove_clones(RUN_PRUNE)
                assert eng.tracks_count()[0] == n0[0] - len(eng.tracks_dropped()) and eng.n_clones == 36
        print(f"resident run: {updates} updates, {wide_updates} with a track of more than 32 views, worst dx {worst['dx']:.2e} P+ {worst['P']:.2e}", flush=True)
        assert updates >= 5 and wide_updates >= 5
        assert sorted(eng.load_tracks_where().tolist()) == [11, 12] and eng.n_clones == 41
        assert len(eng.track(11)["slots"]) == 41


# ---- 7: without the flag nothing moved ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_track", [30, 32])
def test_narrow_stores_are_as_they_were(max_track):
    """`test_a_track_of_31_views_equals_the_host_batch` of tests/test_gpu_tracks.py on both narrow limits, with and without
    the flag (which changes nothing there): the 32-lane instantiations of the per-row kernels."""
    from msckf_amd.api import UpdateEngine
    M = min(max_track, 31)
    N = M
    p, uv = ws.small(N, 5, seed=9)
    ids = [4, 8, 15, 16, 23]
    views = [list(range(M)), list(range(0, M, 3)), list(range(N - 11, N)), [0, N - 1], list(range(5, 17))]
    lost, tracked = np.ones(5, np.int32), np.array([len(v) for v in views], np.int32)
    params = _params()
    kw = dict(max_clones=N, max_features=16, max_track=max_track)
    outs = []
    for flag in (False, True):
        with UpdateEngine(wide_store=flag, **kw) as eng, UpdateEngine(**kw) as eng_b:
            ws.grow(eng, p, uv, views, ids)
            assert len(eng.track(4)["slots"]) == M
            _, b = ws.store_batch(eng, ids)
            door = ws.host_door(eng_b, b, eng.covariance(), p.cam_R, p.cam_t, p.gravity, p.K, p.sigma, lost, tracked, params)
            sel, res, _ = _through_the_store(eng, ids, lost, tracked, params, p.K)
            assert sel.valid.all() and res.status == 0 and eng.debug_split()["long_tracks"] > 0
            ws.same_through_both_doors(sel, res, door[0], door[1], (max_track, flag))
            eng.remove_clones([0, 7])                                # the 32-lane drop: 4 loses two views, its anchor goes
            t = eng.track(4)
            assert t["slots"].tolist() == list(range(M - 2)) and t["anchor_slot"] == -1
            outs.append((sel, res, t))
    ws.same_through_both_doors(outs[0][0], outs[0][1], outs[1][0], outs[1][1], "flag on a narrow context")
    assert all(np.array_equal(outs[0][2][k], outs[1][2][k]) for k in outs[0][2])


def test_a_narrow_store_holds_32_views_and_loads_31():
    """`max_track` = 32 keeps its meaning: rows of 32 views, batch tracks of 31."""
    p, uv = ws.small(32, 2, seed=10)
    from msckf_amd.api import UpdateEngine
    with UpdateEngine(max_clones=33, max_features=4, max_track=32) as eng:
        ws.grow(eng, p, uv, [list(range(32)), list(range(1, 32))], [1, 2])
        assert len(eng.track(1)["slots"]) == 32
        assert _code(eng.load_tracks, [1], [1], [32]) == _ffi.ERR_ARG
        eng.load_tracks([2], [1], [31])
        eng.augment(ws.J15, p.cam_R[-1], p.cam_t[-1] + 0.15)
        assert _code(eng.tracks_observe, [1], uv[:1, 0], [0.5]) == _ffi.ERR_ARG       # the full row


# ---- 8: error paths ----------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_wide_store_as_it_was():
    p, uv = ws.small(34, 4, seed=71)
    ids = [1, 2, 3]
    views = [list(range(34)), list(range(0, 33)), [33]]
    with ws.wide_engine(max_clones=36, max_features=4) as eng:
        assert _code(eng.tracks_observe, [1], uv[0, :1], [1.0]) == _ffi.ERR_STATE         # no state yet
        ws.grow(eng, p, uv, views, ids)
        snap = _snapshot(eng, ids)
        one = uv[:1, 33]
        assert _code(eng.tracks_observe, [-2], one, [1.0]) == _ffi.ERR_ARG                # a bad id
        assert _code(eng.tracks_observe, [1], one, [1.0]) == _ffi.ERR_DUP_SLOT            # already seen in the newest clone
        assert _code(eng.tracks_observe, [2, 2], uv[[1, 1], 33], [1.0, 1.0]) == _ffi.ERR_DUP_SLOT
        assert _code(eng.tracks_observe, [8, 9], uv[[3, 3], 33], [1.0, 1.0]) == _ffi.ERR_ARG      # four rows, three in use
        assert _code(eng.tracks_frame, [8, 9], uv[[3, 3], 33], [1.0, 1.0], p.K, INF, INF) == _ffi.ERR_ARG
        assert _code(eng.tracks_frame, [3], one, [1.0], p.K, INF, INF) == _ffi.ERR_DUP_SLOT
        assert _code(eng.tracks_remove, [2, 77]) == _ffi.ERR_ARG
        assert _code(eng.load_tracks, [1, 77], [1, 1], [2, 2]) == _ffi.ERR_ARG
        assert _code(eng.load_tracks, [1, 1], [1, 1], [2, 2]) == _ffi.ERR_ARG
        assert _code(eng.load_tracks_where, [34]) == _ffi.ERR_ARG
        assert _code(eng.track, 77) == _ffi.ERR_ARG
        assert _same_snapshot(snap, _snapshot(eng, ids))
        eng.tracks_observe([2], uv[1:2, 33], [0.75])                                      # ... and the store still works
        assert len(eng.track(2)["slots"]) == 34 and eng.tracks_count() == (3, 69)
        eng.tracks_reset()
        assert eng.tracks_count() == (0, 0) and _code(eng.track, 1) == _ffi.ERR_ARG
        ws.grow(eng, p, uv, views, ids)                                                   # (set_prior -> msckf_set_state: empties it too)
        assert eng.tracks_count() == (3, 68)
        eng.set_state(p)
        assert eng.tracks_count() == (0, 0)
        eng.load_tracks([], [], [])                                                       # as set_features(F = 0)
        eng.run_select(_params(), p.K)
        eng.run()
        assert eng.result().status == 1


def test_the_f32_combination_is_refused_by_the_library_too():
    import ctypes as C
    lib = _ffi.load()
    for flags, dtype, max_track, want in ((_ffi.FLAG_WIDE_STORE, _ffi.DTYPE_F32, 33, _ffi.ERR_ARG), (_ffi.FLAG_WIDE_STORE, _ffi.DTYPE_F32, 32, 0),
                                          (0, _ffi.DTYPE_F32, 64, 0), (_ffi.FLAG_WIDE_STORE, _ffi.DTYPE_F64, 64, 0)):
        cfg = _ffi.Config(_ffi.ABI_VERSION, 0, 8, 8, max_track, 0, 0, flags, dtype, 0)
        h = C.c_void_p()
        rc = lib.msckf_create(C.byref(h), C.byref(cfg))
        assert rc == want, (flags, dtype, max_track, rc)
        if rc == 0:
            lib.msckf_destroy(h)
