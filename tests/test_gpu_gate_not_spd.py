"""The gate's not-SPD verdict (gate byte 2, msckf_stats.not_spd) on every k_feature instance and every consumer of the byte.

A track whose gate matrix S_j = H_o P H_o^T + sigma^2 I meets a pivot that is not > 0 is dropped BEFORE the chi-square test,
counted in not_spd and not in n_rejected, and the update is that of the batch without it (include/msckf_mi355x.h, next to
not_spd).  The reference does otherwise -- it inverts whatever S_j it gets (MSCKF.py:561-568) --, so the expected result of
every case is oracle.update on the GOOD tracks alone, never the oracle on the whole batch.

The batches are failing_batches.GATE_CASES: one clone slot a of the prior cut off and its block set to -I; the tracks that
see clone a are bad (lambda_min(S_j) <= -10 sigma^2), the others good (>= 0.5 sigma^2), nothing in between
(test_failing_batches.py pins that on the CPU, and which kernel form each case reaches).

  forms      <24> (k24), <32> (k32), <64> chunked (k64: views out of slot order keep a long track whole), <64, true, 4>
             (split, remainder rows as they are and through their own tree), <64, true> (the same in a child process with
             MSCKF_SPLIT_MW_MAX=0) -- each through update_problem (direct result, the gate's host mirror) and through
             load / run / result, with the blocks of a split track carrying their track's byte; plan="tree" for the merge
             tree's leaves (k_fold; k_fold_g needs a node of more than 186 columns: tree_wide, N = 34)
  consumers  all tracks bad (no-op), run_select in front (bytes 0, 1, 2, 3 in one batch) + replan, dtype f32, commit and go
             on (+ remove_clones of the bad clone), 4 logical shards in the three exchange formats with a shard of bad tracks
             only, the track store's emit path
  non-finite one track with a NaN / +inf observation (S_j is sound, gamma is NaN: chi-square side, n_rejected) or a NaN
             inverse-depth point (S_j is NaN: byte 2, not_spd) on the ORIGINAL positive-definite prior; every other track,
             dx and P+ as the oracle gives them without that track

Tolerances: dx, P+ 1e-8 relative (BASELINE.json); dtype f32 1e-4 / 1e-5 (test_gpu_f32.py); gamma of the good tracks
rtol 1e-9, atol 1e-12 (test_gate_statistic_of_long_tracks).  Errors observed on one MI355X: DESIGN.md section 5."""
import os
import subprocess
import sys

import numpy as np
import pytest

import failing_batches as fb
from conftest import ROOT, rel_err
from msckf_amd import synth
from oracle import msckf_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 1e-8
TOL_F32 = (1e-4, 1e-5)
GAMMA_TOL = dict(rtol=1e-9, atol=1e-12)

_CASES = {}


def case(name):
    """(prob, bad mask, indices of the good tracks, oracle.update on them) -- computed once, never changed."""
    if name not in _CASES:
        prob, bad = fb.gate_case(name)
        good = np.nonzero(~bad)[0]
        _CASES[name] = (prob, bad, good, oracle.update(prob.take(good), dense_noise=False) if len(good) else None)
    return _CASES[name]


def engine(**kw):
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=31, max_features=256, max_track=31)
    args.update(kw)
    return UpdateEngine(**args)


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


def scatter(F, idx, values, fill=0):
    out = np.full(F, fill, dtype=np.uint8)
    out[idx] = values
    return out


def p_error(P_new, P_ref, clone):
    """P+ against the oracle's.  The -I block of the cut-off clone dominates the norm of P (2.4 against entries of 1e-3), so a
    relative error over the whole matrix would let the part the update works on be wrong by four more digits: the error is
    taken over P+ WITHOUT that clone's rows and columns, and those -- which no good track's row touches -- must come back bit
    for bit (the oracle's do: test_failing_batches.py)."""
    if clone is None:
        return rel_err(P_new, P_ref)
    i = 15 + 6 * clone
    keep = np.r_[0:i, i + 6:P_ref.shape[0]]
    assert np.array_equal(P_new[i:i + 6], P_ref[i:i + 6]) and np.array_equal(P_new[:, i:i + 6], P_ref[:, i:i + 6])
    return max(rel_err(P_new[np.ix_(keep, keep)], P_ref[np.ix_(keep, keep)]), rel_err(P_new, P_ref))


def check_result(res, prob, n_bad, good, ref, what, tol=(TOL, TOL), n_unselected=0, clone=None):
    """status, mask, the four counters, dx and P+ against the oracle on the good tracks."""
    n_acc = int(ref["accepted"].sum())
    e_dx, e_P = rel_err(res.dx, ref["dx"]), p_error(res.P_new, ref["P_new"], clone)
    print("%s: dx %.2e P+ %.2e | accepted %d rejected %d not_spd %d of %d"
          % (what, e_dx, e_P, res.stats["n_accepted"], res.stats["n_rejected"], res.stats["not_spd"], prob.F), flush=True)
    assert res.status == ref["status"] == 0, what
    assert np.array_equal(res.accepted, scatter(prob.F, good, ref["accepted"])), what
    assert res.stats["n_accepted"] == n_acc, what
    assert res.stats["n_rejected"] == len(good) - n_acc == ref["n_rejected"] == res.n_rejected, what
    assert res.stats["not_spd"] == n_bad, what
    if "n_features" in res.stats and res.stats["n_features"]:
        assert res.stats["n_features"] == prob.F - n_unselected, what
    assert e_dx < tol[0] and e_P < tol[1], (what, e_dx, e_P)


def check_gate(e, prob, bad, good, ref, what, split=True):
    """gamma of the good tracks, the byte of every track, and the bytes the blocks of split tracks inherited."""
    gam, _ = e.debug_gate()
    err = np.abs(gam[good] - ref["gamma"]) / np.maximum(np.abs(ref["gamma"]), 1e-300)
    print("%s: gamma worst relative error %.2e" % (what, err.max()), flush=True)
    np.testing.assert_allclose(gam[good], ref["gamma"], **GAMMA_TOL)
    codes, block_codes, block_track = e.gate_codes()
    assert np.array_equal(codes, scatter(prob.F, good, ref["accepted"], fill=2)), what
    long = fb.long_tracks(prob) if split else np.zeros(prob.F, dtype=bool)
    assert e.debug_split()["long_tracks"] == int(long.sum()), what
    if long.any():
        assert len(block_codes) == e.debug_split()["entries"] - prob.F > 0
        assert set(block_track.tolist()) == set(np.nonzero(long)[0].tolist())
        assert np.array_equal(block_codes, codes[block_track]), what       # a block carries its track's byte
    else:
        assert len(block_codes) == 0


def run_form(e, name, direct_rows=-1, tol=(TOL, TOL), what=None, split=True):
    """One case through the one-shot call and through load / run / result on the resident state (split=False: the engine's
    plan splits no track)."""
    prob, bad, good, ref = case(name)
    what = what or name
    n_bad, a = int(bad.sum()), fb.GATE_CASES[name][4]
    e.set_rem_direct_rows(direct_rows)
    try:
        res = e.update_problem(prob)
        check_result(res, prob, n_bad, good, ref, what + " update_problem", tol, clone=a)
        check_gate(e, prob, bad, good, ref, what + " update_problem", split)
        assert res.stats["stacked_rows"] == ref["H_X"].shape[0]
        long = fb.long_tracks(prob) if split else np.zeros(prob.F, dtype=bool)
        if long.any():
            s = e.debug_split()
            assert s["remainder_mode"] == (1 if direct_rows < 0 else 2), s
            assert (s["remainder_rows_cap"] + 15) // 16 == fb.remainder_blocks(prob, long)
            assert (long & bad).any() and (long & ~bad).any()
        e.load(prob)
        e.run()
        res2 = e.result()
        check_result(res2, prob, n_bad, good, ref, what + " load/run/result", tol, clone=a)
        check_gate(e, prob, bad, good, ref, what + " load/run/result", split)
        if tol == (TOL, TOL):                                        # (the same kernels on the same numbers)
            assert rel_err(res2.dx, res.dx) < 1e-10 and rel_err(res2.P_new, res.P_new) < 1e-11
    finally:
        e.set_rem_direct_rows(-1)


# ---- 2. every k_feature form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,direct_rows", [("k24", -1), ("k32", -1), ("k64", -1), ("split", -1), ("split", 0)],
                         ids=["k24", "k32", "k64_unsplit", "split_rows", "split_tree"])
def test_bad_tracks_are_dropped_and_reported(eng, name, direct_rows):
    run_form(eng, name, direct_rows)


@pytest.mark.parametrize("name", ["k64", "tree_wide"])
def test_tree_plan(name):
    """plan="tree": every track, whatever its length, through the merge tree's leaves -- k_fold up to 186 columns (k64, N = 20),
    k_fold_g beyond (tree_wide, N = 34: the one case of this file past 31 clones; leaves of up to 1024 rows, so that one holds
    tracks from both ends of the window and is 204 columns wide)."""
    N = case(name)[0].N
    with engine(max_clones=N, max_features=64, plan="tree", leaf_rows=1024 if name == "tree_wide" else 0) as e:
        run_form(e, name, what=name + " tree plan", split=False)
        s = e.debug_split()
        assert s["band_plan"] == 0 and s["long_tracks"] == 0, s


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import msckf_amd
import test_gpu_gate_not_spd as t
with t.engine() as e:
    t.run_form(e, "split", -1, what="split, one wavefront per track")
    t.run_form(e, "split", 0, what="split, one wavefront per track, remainder tree")
print("FORM_OK")
"""


def test_split_form_with_one_wavefront_per_track():
    """k_feature<64, true>: MSCKF_SPLIT_MW_MAX is read once per process."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MSCKF_SPLIT_MW_MAX="0"), cwd=ROOT)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "FORM_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- 3. the consumers ------------------------------------------------------------------------------------------------------
def test_every_track_bad_is_a_no_op(eng):
    prob, bad, good, _ = case("all_bad")
    assert bad.all() and len(good) == 0
    res = eng.update_problem(prob)
    for what in ("update_problem", "load/run/result"):
        assert res.status == 1, what
        assert res.stats["not_spd"] == prob.F and res.stats["n_rejected"] == 0 and res.stats["n_accepted"] == 0, (what, res.stats)
        assert res.n_rejected == 0 and not res.accepted.any()
        assert not res.dx.any() and np.array_equal(res.P_new, prob.P), what
        assert np.array_equal(eng.gate_codes()[0], np.full(prob.F, 2, dtype=np.uint8))
        if what == "update_problem":
            eng.load(prob)
            eng.run()
            res = eng.result()
    assert eng.commit_covariance() == 1
    assert np.array_equal(eng.covariance(), prob.P)


def test_mixed_with_selection_holds_all_four_bytes(eng):
    """set_tracks + run_select in front: not selected (3), not SPD (2), rejected (0), accepted (1) in one batch."""
    prob, bad, _, _ = case("mixed")
    tracks = fb.gate_select_tracks(prob)
    sel, valid, idx, ref = fb.gate_selected(prob, tracks, bad)
    n_bad, n_unsel = int((valid & bad).sum()), int((~valid).sum())
    expected = scatter(prob.F, idx, ref["accepted"], fill=3)
    expected[valid & bad] = 2
    assert all((expected == b).any() for b in (0, 1, 2, 3))
    eng.load(prob)
    eng.set_tracks(tracks)
    eng.run_select(fb.GATE_SELECT, prob.K)
    eng.run()
    first = eng.result()
    assert np.array_equal(eng.selection().flags & 1, valid.astype(np.uint8))
    check_result(first, prob, n_bad, idx, ref, "mixed, run_select", n_unselected=n_unsel, clone=fb.GATE_CASES["mixed"][4])
    assert first.stats["n_features"] == int(valid.sum())
    assert np.array_equal(eng.gate_codes()[0], expected)
    gam, _ = eng.debug_gate()
    np.testing.assert_allclose(gam[idx], ref["gamma"], **GAMMA_TOL)
    eng.replan()                                                  # the plan over the valid tracks only
    eng.run()
    again = eng.result()
    check_result(again, prob, n_bad, idx, ref, "mixed, replan", n_unselected=n_unsel, clone=fb.GATE_CASES["mixed"][4])
    assert np.array_equal(eng.gate_codes()[0], expected)
    assert rel_err(again.dx, first.dx) < 1e-10 and rel_err(again.P_new, first.P_new) < 1e-11
    eng.clear_selection()


@pytest.mark.parametrize("name", ["k24", "split"])
def test_f32_mode(name):
    with engine(dtype="f32") as e:
        run_form(e, name, -1, TOL_F32, what=name + " f32")


def test_commit_and_go_on():
    """After the split case: commit, the same batch on the committed prior (the -I block is still there), then the bad clone
    removed: every gate matrix is SPD again and the oracle on the WHOLE batch is the reference."""
    prob, bad, good, ref = case("split")
    a = fb.GATE_CASES["split"][4]
    n_bad = int(bad.sum())
    with engine() as e:
        e.load(prob)
        P = prob.P
        for step in (1, 2):
            if step == 2:
                e.set_features(prob)
            e.run()
            refs = ref if step == 1 else oracle.update(synth.UpdateProblem(**{**prob.__dict__, "P": P}).take(good), dense_noise=False)
            res = e.result()
            check_result(res, prob, n_bad, good, refs, "commit and go on, update %d" % step, clone=a)
            assert e.commit_covariance() == 0
            assert np.array_equal(e.covariance(), res.P_new)
            P = refs["P_new"]
        i = 15 + 6 * a
        assert np.array_equal(e.covariance()[i:i + 6, i:i + 6], -np.eye(6))
        e.remove_clones([a])
        vp, uv, sl, left = fb.without_clone(prob, a)
        keep = np.delete(np.arange(prob.N), a)
        q = synth.UpdateProblem(**{**prob.__dict__, "P": oracle.remove_clones_covariance(P, [a]), "cam_R": prob.cam_R[keep],
                                   "cam_t": prob.cam_t[keep], "cam_R0": prob.cam_R0[keep], "cam_t0": prob.cam_t0[keep],
                                   "view_ptr": vp, "obs_uv": uv, "obs_slot": sl}).take(left)
        ref3 = oracle.update(q, dense_noise=False)
        assert rel_err(e.covariance(), q.P) < TOL
        e.set_features(q)
        e.run()
        res3 = e.result()
        check_result(res3, q, 0, np.arange(q.F), ref3, "commit and go on, clone %d removed" % a)
        assert res3.stats["not_spd"] == 0 and not (e.gate_codes()[0] == 2).any()


def _bad_last(prob, bad, sprinkle):
    """The batch reordered: the good tracks with `sprinkle` bad ones among them, then the other bad tracks in one run."""
    good, b = np.nonzero(~bad)[0], np.nonzero(bad)[0]
    third = len(good) // 3
    order = np.concatenate([good[:third], b[:sprinkle // 2], good[third:2 * third], b[sprinkle // 2:sprinkle], good[2 * third:],
                            b[sprinkle:]])
    return prob.take(order), bad[order]


def _shared(e, prob, bad, good, ref, what, clone):
    """msckf_get_shared_result as every rank reads it after the broadcast (the same result range): twice, the same answer."""
    out = [e.shared_result() for _ in range(2)]
    for res in out:
        check_result(res, prob, int(bad.sum()), good, ref, what, clone=clone)
    assert np.array_equal(out[0].accepted, out[1].accepted) and out[0].stats["not_spd"] == out[1].stats["not_spd"]
    assert np.array_equal(out[0].dx, out[1].dx) and np.array_equal(out[0].P_new, out[1].P_new)


def _record_gate_bytes(rec, N, n):
    return int(round(rec[N])), np.ascontiguousarray(rec[N + 1:N + 1 + (n + 7) // 8]).view(np.uint8)[:n]


def test_logical_shards_group_records():
    """The calls of test_shipped_merge_path_logical_shards on the (30, 200, 10) case, 4 shards, the last of bad tracks only."""
    from msckf_amd.shard import shard_group_flags
    p0, b0, _, _ = case("mixed")
    prob, bad = _bad_last(p0, b0, 4)
    good = np.nonzero(~bad)[0]
    ref = oracle.update(prob.take(good), dense_noise=False)
    n_tail = int(bad.sum()) - 4
    cut = prob.F - n_tail
    shards = [(0, cut // 3), (cut // 3, 2 * cut // 3), (2 * cut // 3, cut), (cut, prob.F)]
    assert bad[cut:].all() and bad[:cut].sum() == 4
    bounds = np.array([s[0] for s in shards] + [prob.F], dtype=np.int32)
    with engine(max_clones=prob.N + 3, max_features=128, max_track=10) as e:
        assert e.band_ok(prob)
        e.set_group_exchange(True)
        e.set_exchange_span(e.max_span(prob))
        e.set_exchange_mask(bounds)
        count, recv = None, 0
        for r, (lo, hi) in enumerate(shards):
            e.load(prob.subset(lo, hi))
            if count is None:
                count = e.group_record_doubles()
                recv = e.comm_buffer(count * (len(shards) + 1) + 8)
            assert e.group_record_doubles() == count
            e.run_compress()
            e.export_groups(dst_ptr=recv + 8 * count * r, count=False)
        recs = e.comm_get(recv, count * len(shards)).reshape(len(shards), count)
        expected = scatter(prob.F, good, ref["accepted"], fill=2)
        for r, (lo, hi) in enumerate(shards):
            n_acc, gate = _record_gate_bytes(recs[r], prob.N, hi - lo)
            assert np.array_equal(gate, expected[lo:hi]) and n_acc == int((expected[lo:hi] == 1).sum()), r
        n_acc, gate = _record_gate_bytes(recs[3], prob.N, n_tail)
        assert n_acc == 0 and (gate == 2).all()                      # the shard of bad tracks: count 0, gate bytes 2
        e.set_state(prob)
        flags = shard_group_flags(prob, shards)
        for it in range(2):                                          # the second call reuses the cached merge plan
            e.merge_groups_flags(recv, len(shards), flags)
            _shared(e, prob, bad, good, ref, "group records, merge %d" % it, fb.GATE_CASES["mixed"][4])
        e.set_exchange_mask(None)
        e.set_exchange_span(0)
        e.set_group_exchange(False)


def test_logical_shards_split_records():
    """The calls of RcclShardedUpdate with split records on the long-track case: two of the four shards hold bad tracks only."""
    p0, b0, _, _ = case("split")
    prob, bad = _bad_last(p0, b0, 10)
    good = np.nonzero(~bad)[0]
    ref = oracle.update(prob.take(good), dense_noise=False)
    cut = prob.F - (int(bad.sum()) - 10)
    mid = (cut + prob.F) // 2
    shards = [(0, cut // 2), (cut // 2, cut), (cut, mid), (mid, prob.F)]
    assert bad[cut:].all() and bad[:cut].sum() == 10
    long = fb.long_tracks(prob)
    assert long[cut:mid].any() and long[mid:].any() and (long & ~bad).any()
    bounds = np.array([s[0] for s in shards] + [prob.F], dtype=np.int32)
    S = len(shards)
    with engine(max_features=128) as e:
        rule = e.exchange_split_rule(prob, shards)
        assert rule["split"]
        e.set_group_exchange(True)
        e.set_exchange_split(rule["rows"], rule["total"])
        e.set_exchange_span(rule["span"])
        e.set_exchange_mask(bounds)
        try:
            count, recv = None, 0
            for r, (lo, hi) in enumerate(shards):
                e.load(prob.subset(lo, hi))
                if count is None:
                    count = e.group_record_doubles()
                    recv = e.comm_buffer(count * (S + 1) + 8)
                assert e.group_record_doubles() == count
                e.run_compress()
                assert e.debug_split()["long_tracks"] == int(long[lo:hi].sum())
                e.export_groups(dst_ptr=recv + 8 * count * r, count=False)
            rem = 1 + rule["rows"] * (6 * prob.N + 1)
            recs = e.comm_get(recv, count * S).reshape(S, count)
            expected = scatter(prob.F, good, ref["accepted"], fill=2)
            for r, (lo, hi) in enumerate(shards):
                n_acc, gate = _record_gate_bytes(recs[r], prob.N, hi - lo)
                rows = int(np.ascontiguousarray(recs[r, count - rem:count - rem + 1]).view(np.int32)[1])
                assert np.array_equal(gate, expected[lo:hi]) and n_acc == int((expected[lo:hi] == 1).sum()), r
                assert (rows > 0) == bool(((expected[lo:hi] == 1) & long[lo:hi]).any()), (r, rows)
                if r >= 2:
                    assert n_acc == 0 and rows == 0 and (gate == 2).all()   # bad tracks only: no count, no remainder row
            e.set_state(prob)
            for it in range(2):
                e.merge_groups_flags(recv, S, rule["flags"])
                _shared(e, prob, bad, good, ref, "split records, merge %d" % it, fb.GATE_CASES["split"][4])
        finally:
            e.set_exchange_mask(None)
            e.set_exchange_split(0)
            e.set_exchange_span(0)
            e.set_group_exchange(False)


def test_logical_shards_root_block_fallback():
    """Views out of slot order: the rule refuses split records, the ranks ship root blocks, their accepted counts and their gate
    bytes through host memory (RcclShardedUpdate.step's else-branch) -- the bytes as k_feature wrote them, 2 included."""
    p0, b0, _, _ = case("k64")
    prob, bad = _bad_last(p0, b0, 4)
    good = np.nonzero(~bad)[0]
    ref = oracle.update(prob.take(good), dense_noise=False)
    cut = prob.F - (int(bad.sum()) - 4)
    shards = [(0, cut // 3), (cut // 3, 2 * cut // 3), (2 * cut // 3, cut), (cut, prob.F)]
    assert bad[cut:].all()
    bounds = np.array([s[0] for s in shards] + [prob.F], dtype=np.int32)
    with engine(max_features=64) as e:
        assert not e.exchange_split_rule(prob, shards)["split"] and not e.band_ok(prob)
        e.set_group_exchange(False)
        e.set_exchange_span(0)
        e.set_exchange_mask(bounds)
        try:
            blocks, total = [], 0
            allg = np.zeros((prob.F + 7) // 8 * 8, dtype=np.uint8)
            for r, (lo, hi) in enumerate(shards):
                e.load(prob.subset(lo, hi))
                e.run_compress()
                blk, n = e.export_block()
                allg[lo:hi] = e.gate_bytes()
                if r == 3:
                    assert n == 0 and (allg[lo:hi] == 2).all()
                blocks.append(blk)
                total += n
            assert total == int(ref["accepted"].sum())
            e.set_state(prob)
            e.merge_gain(np.stack(blocks), total)
            e.comm_put(e.device_pointer(6), allg.view(np.float64))
            _shared(e, prob, bad, good, ref, "root blocks", fb.GATE_CASES["k64"][4])
        finally:
            e.set_exchange_mask(None)


def test_from_the_track_store():
    """The <24> case grown clone by clone in the track store and loaded by msckf_tracks_load: the emit path (the raw image never
    visits the host) with run_select in front, against the oracle chain on what the store holds."""
    p0, bad, _, _ = case("k24")
    N, F = p0.N, p0.F
    ids = 100 + 3 * np.arange(F)
    params = synth.SelectParams(min_frames_lost=1, min_frames_tracked=2, use_parallax=False, min_parallax_deg=0.0)
    with engine(max_clones=16, max_features=64, max_track=10) as e:
        e.set_prior(np.eye(15) * 0.1, p0.gravity, p0.K, p0.sigma)
        for s in range(N):
            e.augment(np.zeros((6, 15)), p0.cam_R[s], p0.cam_t[s])
            at = np.nonzero(np.asarray(p0.obs_slot) == s)[0]
            js = np.searchsorted(p0.view_ptr, at, side="right") - 1
            e.tracks_observe(ids[js], p0.obs_uv[at], 0.5 + 0.005 * np.arange(len(js)))
        e.import_covariance(p0.P)
        tr = [e.track(int(i)) for i in ids]
        assert all(np.array_equal(t["slots"], p0.obs_slot[p0.view_ptr[j]:p0.view_ptr[j + 1]]) for j, t in enumerate(tr))
        cat = lambda k, w: np.concatenate([t[k].reshape(-1, w) for t in tr])
        held = synth.UpdateProblem(**{**p0.__dict__, "obs_uv": cat("uv", 2), "idp_base": np.array([t["idp_base"] for t in tr]),
                                      "idp_m": np.array([t["idp_m"] for t in tr]), "idp_rho": np.array([t["idp_rho"] for t in tr])})
        lost = np.ones(F, np.int32)
        tracked = np.diff(p0.view_ptr).astype(np.int32)
        tracks = synth.TrackTable(line_base=cat("line_base", 3), line_dir=cat("dir", 3), line_conf=cat("conf", 1).reshape(-1),
                                  lost_for=lost, tracked_for=tracked)
        sel, valid, idx, ref = fb.gate_selected(held, tracks, bad, params)
        assert valid.all()
        lam = fb.gate_lambda(synth.UpdateProblem(**{**held.__dict__, "idp_m": sel["idp_m"], "idp_rho": sel["idp_rho"]}))
        assert (lam[bad] <= -10.0).all() and (lam[~bad] >= 0.5).all()   # the store's refreshed points classify the same way
        e.load_tracks(ids, lost, tracked)
        e.run_select(params, p0.K)
        e.run()
        res = e.result()
        check_result(res, held, int(bad.sum()), idx, ref, "track store", clone=fb.GATE_CASES["k24"][4])
        assert np.array_equal(e.gate_codes()[0], scatter(F, idx, ref["accepted"], fill=2))


# ---- 4. non-finite tracks --------------------------------------------------------------------------------------------------
# variant: (what is corrupted, the byte k_feature must write, the counter the track lands in).  An observation enters the
# residual alone: S_j is sound, every pivot positive, gamma = NaN fails `gam <= chi2`: byte 0, n_rejected.  The inverse-depth
# point enters H_f and H_x: S_j is NaN, the first pivot fails `piv > 0`: byte 2, not_spd.
NONFINITE = {
    "nan_uv": ("obs_uv", np.nan, 0, "n_rejected"),
    "inf_uv": ("obs_uv", np.inf, 0, "n_rejected"),
    "nan_rho": ("idp_rho", np.nan, 2, "not_spd"),
    "nan_m": ("idp_m", np.nan, 2, "not_spd"),
}
_CLEAN = {}


def _clean(name):
    """The case's batch on its ORIGINAL positive-definite prior, its oracle result, the track to corrupt (accepted; long in the
    split case) and the oracle on the batch without it."""
    if name not in _CLEAN:
        N, F, M, seed, a, kw = fb.GATE_CASES[name][:6]
        prob = synth.make_problem(N, F, M, seed=seed, **kw)
        ref = oracle.update(prob, dense_noise=False)
        long = fb.long_tracks(prob)
        cand = np.nonzero((ref["accepted"] == 1) & (long if long.any() else True))[0]
        j = int(cand[len(cand) // 2])
        others = np.delete(np.arange(F), j)
        _CLEAN[name] = (prob, j, others, oracle.update(prob.take(others), dense_noise=False))
    return _CLEAN[name]


@pytest.mark.parametrize("variant", sorted(NONFINITE))
@pytest.mark.parametrize("name", ["k24", "split"])
def test_one_non_finite_track_is_dropped(eng, name, variant):
    prob, j, others, ref = _clean(name)
    field, value, byte, counter = NONFINITE[variant]
    arr = np.array(getattr(prob, field), dtype=np.float64, copy=True)
    if field == "obs_uv":
        arr[int(prob.view_ptr[j]) + 1, 0] = value                 # the second view's u
    elif field == "idp_rho":
        arr[j] = value
    else:
        arr[j, 1] = value
    q = synth.UpdateProblem(**{**prob.__dict__, field: arr})
    res = eng.update_problem(q)
    n_acc = int(ref["accepted"].sum())
    e_dx, e_P = rel_err(res.dx, ref["dx"]), rel_err(res.P_new, ref["P_new"])
    codes = eng.gate_codes()[0]
    print("%s %s: byte %d, n_rejected %d, not_spd %d, dx %.2e P+ %.2e" % (name, variant, codes[j], res.stats["n_rejected"],
                                                                          res.stats["not_spd"], e_dx, e_P), flush=True)
    assert res.status == 0 and res.accepted[j] == 0 and codes[j] == byte
    assert np.array_equal(res.accepted[others], ref["accepted"]) and np.array_equal(codes[others], ref["accepted"])
    assert res.stats["n_accepted"] == n_acc
    assert res.stats["n_rejected"] == len(others) - n_acc + (counter == "n_rejected")
    assert res.stats["not_spd"] == (counter == "not_spd")
    gam, _ = eng.debug_gate()
    np.testing.assert_allclose(gam[others], ref["gamma"], **GAMMA_TOL)
    assert np.isfinite(res.dx).all() and np.isfinite(res.P_new).all()
    assert e_dx < TOL and e_P < TOL, (e_dx, e_P)
    if fb.long_tracks(prob).any():
        codes, block_codes, block_track = eng.gate_codes()
        assert np.array_equal(block_codes, codes[block_track]) and (block_track == j).any()
