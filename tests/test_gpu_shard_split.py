"""Split records: a sharded update of a batch with long tracks through the group exchange -- every rank splits
its long tracks as one GPU does (narrow blocks in the group slots, remainder rows in a section of the record), rank 0
folds the groups and takes the collected remainder rows as K6-K7's second source.  The calls of
`RcclShardedUpdate.load / step / result` with S logical shards on ONE engine, checked against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err
from msckf_amd import synth
from oracle import msckf_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 1e-8


def _spans(prob):
    vp = np.asarray(prob.view_ptr)
    slots = np.asarray(prob.obs_slot).reshape(-1)
    if prob.F == 0:
        return np.zeros(0, dtype=np.int64)
    return np.maximum.reduceat(slots, vp[:-1]) - np.minimum.reduceat(slots, vp[:-1]) + 1


def _split_merge(e, prob, shards, ref, tol_dx=TOL, tol_P=TOL, calls=2):
    """Every shard's split record copied (in HBM) into slot r of the exchange buffer, rank 0's merge with the rule's
    flags, the shared result range read as every rank reads it after the broadcast.  Returns the last result."""
    rule = e.exchange_split_rule(prob, shards)
    assert rule["split"]
    S = len(shards)
    bounds = np.array([sh[0] for sh in shards] + [shards[-1][1]], dtype=np.int32)
    e.set_group_exchange(True)
    e.set_exchange_split(rule["rows"], rule["total"])
    e.set_exchange_span(rule["span"])
    e.set_exchange_mask(bounds)
    spans = _spans(prob)
    count, recv = None, 0
    try:
        for r, (lo, hi) in enumerate(shards):
            e.load(prob.subset(lo, hi))
            if count is None:
                count = e.group_record_doubles()
                recv = e.comm_buffer(count * (S + 1) + 8)
            assert e.group_record_doubles() == count
            e.run_compress()
            n_long = int((spans[lo:hi] > 10).sum())
            if hi > lo:
                assert e.debug_split()["long_tracks"] == n_long
            e.export_groups(dst_ptr=recv + 8 * count * r, count=False)
        # the remainder section: present, its row count where the record's layout puts it
        rem = 1 + rule["rows"] * (6 * prob.N + 1)
        recs = e.comm_get(recv, count * S).reshape(S, count)
        rows = [int(np.ascontiguousarray(recs[r, count - rem:count - rem + 1]).view(np.int32)[1]) for r in range(S)]
        acc = ref["accepted"].astype(bool)
        for r, (lo, hi) in enumerate(shards):
            assert 0 <= rows[r] <= rule["rows"]
            assert (rows[r] > 0) == bool((acc[lo:hi] & (spans[lo:hi] > 10)).any())
        e.set_state(prob)
        out = []
        for _ in range(calls):                                # the second call reuses the cached merge plan
            e.merge_groups_flags(recv, S, rule["flags"])
            res = e.shared_result()
            assert res.status == ref["status"]
            assert np.array_equal(res.accepted, ref["accepted"])
            assert res.n_rejected == prob.F - int(ref["accepted"].sum())
            if ref["status"] == 0:
                assert rel_err(res.dx, ref["dx"]) < tol_dx, rel_err(res.dx, ref["dx"])
                assert rel_err(res.P_new, ref["P_new"]) < tol_P, rel_err(res.P_new, ref["P_new"])
            out.append(res)
        for res in out[1:]:
            assert np.array_equal(res.dx, out[0].dx) and np.array_equal(res.P_new, out[0].P_new)
        return out[-1]
    finally:
        e.set_exchange_mask(None)
        e.set_exchange_split(0)
        e.set_exchange_span(0)
        e.set_group_exchange(False)


def _root_block_merge(e, prob, shards, ref):
    """The fallback exchange of `RcclShardedUpdate.step`: root blocks per shard, rank 0's `merge_gain`."""
    e.set_group_exchange(False)
    blocks, total = [], 0
    for lo, hi in shards:
        e.load(prob.subset(lo, hi))
        e.run_compress()
        blk, n = e.export_block()
        blocks.append(blk)
        total += n
    e.set_state(prob)
    e.merge_gain(np.stack(blocks), total)
    res = e.result()
    assert res.status == ref["status"]
    if ref["status"] == 0:
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL


def _engine(N, F, M, **kw):
    from msckf_amd.api import UpdateEngine
    return UpdateEngine(max_clones=N, max_features=max(F, 8), max_track=M, **kw)


FRAME = {"variable_tracks": True, "min_track": 2, "outlier_fraction": 0.1, "outlier_px": 400.0}


@pytest.mark.parametrize("S", [2, 4, 8])
def test_frame_of_the_reference_size(S):
    """(30, 300, ~U[2, 30]) with 10 % outliers: ~1600 remainder rows, the early update beside the group folds."""
    from msckf_amd.shard import partition_features
    prob = synth.make_problem(30, 300, 30, seed=81, **FRAME)
    ref = oracle.update(prob, dense_noise=False)
    with _engine(30, 300, 30) as e:
        _split_merge(e, prob, partition_features(prob.view_ptr, S), ref)


@pytest.mark.parametrize("S", [2, 8])
def test_few_long_among_many_short(S):
    """1990 ten-view + 10 thirty-view tracks: 90 remainder rows, taken inside the root's launch."""
    from msckf_amd.shard import partition_features
    prob = synth.few_long_tracks_problem(30, 2000, 10, 10, seed=82)
    ref = oracle.update(prob, dense_noise=False)
    with _engine(30, 2000, 30) as e:
        _split_merge(e, prob, partition_features(prob.view_ptr, S), ref)


def test_many_remainder_row_blocks():
    """(30, 600, ~U[2, 30]) over 4 shards: well over 20 row blocks of remainder rows."""
    from msckf_amd.shard import partition_features
    prob = synth.make_problem(30, 600, 30, seed=83, variable_tracks=True, min_track=2)
    ref = oracle.update(prob, dense_noise=False)
    with _engine(30, 600, 30) as e:
        _split_merge(e, prob, partition_features(prob.view_ptr, 4), ref)


def test_shard_with_only_long_tracks_and_one_with_none():
    prob = synth.few_long_tracks_problem(30, 200, 20, 10, seed=84)      # tracks [180, 200) span the window
    ref = oracle.update(prob, dense_noise=False)
    with _engine(30, 200, 30) as e:
        _split_merge(e, prob, [(0, 90), (90, 180), (180, 200)], ref)


def test_every_long_track_fails_the_gate():
    """Remainder count 0 in every record: the merge's second source is empty."""
    from msckf_amd.shard import partition_features
    prob = synth.few_long_tracks_problem(30, 400, 12, 10, seed=85)
    vp = np.asarray(prob.view_ptr)
    uv = prob.obs_uv.copy()
    rng = np.random.default_rng(5)
    for j in range(388, 400):
        a, b = int(vp[j]), int(vp[j + 1])
        uv[a:b] += rng.normal(0.0, 400.0, size=(b - a, 2))
    prob.obs_uv = uv
    ref = oracle.update(prob, dense_noise=False)
    assert not ref["accepted"][388:].any() and ref["accepted"][:388].any()
    with _engine(30, 400, 30) as e:
        _split_merge(e, prob, partition_features(prob.view_ptr, 3), ref)


def test_window_over_33_clones():
    """(50, 300, <= 31 views): the remainder rows through k_gain_stream (not k_gain_dense), the band root in a ring."""
    from msckf_amd.shard import partition_features
    prob = synth.make_problem(50, 300, 31, seed=86, variable_tracks=True, min_track=2)
    ref = oracle.update(prob, dense_noise=False)
    with _engine(50, 300, 31) as e:
        _split_merge(e, prob, partition_features(prob.view_ptr, 4), ref)


def test_f32_mode_on_the_frame():
    from msckf_amd.shard import partition_features
    prob = synth.make_problem(30, 300, 30, seed=87, **FRAME)
    ref = oracle.update(prob, dense_noise=False)
    with _engine(30, 300, 30, dtype="f32") as e:
        _split_merge(e, prob, partition_features(prob.view_ptr, 4), ref, 1e-4, 1e-5)


@pytest.mark.parametrize("case", ["edge_long_tracks", "edge_mixed_spans", "edge_few_long_among_short", "edge_gauge_prior"])
@pytest.mark.parametrize("S", [2, 3])
def test_reference_fixtures(case, S):
    from msckf_amd.shard import partition_features
    prob, ref = load_golden(case)
    ref = {"status": int(ref["status"]), "accepted": ref["accepted"], "dx": ref["dx"], "P_new": ref["P_new"]}
    with _engine(prob.N, prob.F, 31) as e:
        _split_merge(e, prob, partition_features(prob.view_ptr, S), ref)


def test_record_size_without_the_setter():
    """A context on which msckf_set_exchange_split is never called (or set to 0) lays its records out as before."""
    prob = synth.make_problem(30, 300, 30, seed=88, variable_tracks=True, min_track=2)
    with _engine(30, 300, 30) as e:
        e.set_group_exchange(True)
        e.set_exchange_span(10)
        e.load(prob.subset(0, 0))
        base = e.group_record_doubles()
        assert base == 30 + 1 + 30 * 60 * 61
        e.set_exchange_split(100, 300)
        e.load(prob.subset(0, 0))
        assert e.group_record_doubles() == base + 1 + 112 * 181
        e.set_exchange_split(0)
        e.load(prob.subset(0, 0))
        assert e.group_record_doubles() == base


def test_fallbacks_keep_root_blocks():
    """A track with views out of slot order and a batch over the row cap: "not split" from the rule, root blocks, still
    correct.  (Tracks of more than 31 views, which the rule refuses too -- tests/test_exchange_split_rule.py --, no engine
    takes: MAX_TRACK.)"""
    from msckf_amd.shard import partition_features
    unordered = synth.make_problem(24, 60, 24, seed=90, variable_tracks=True, min_track=12)
    vp = unordered.view_ptr
    uv, sl = unordered.obs_uv.copy(), unordered.obs_slot.copy()
    for j in range(0, unordered.F, 2):
        a, b = int(vp[j]), int(vp[j + 1])
        uv[a:b] = uv[a:b][::-1].copy()
        sl[a:b] = sl[a:b][::-1].copy()
    unordered.obs_uv, unordered.obs_slot = uv, sl
    ref = oracle.update(unordered, dense_noise=False)
    shards = partition_features(unordered.view_ptr, 2)
    with _engine(24, 60, 24) as e:
        assert not e.exchange_split_rule(unordered, shards)["split"]
        _root_block_merge(e, unordered, shards, ref)
    prob = synth.make_problem(30, 300, 30, seed=91, variable_tracks=True, min_track=2)
    ref = oracle.update(prob, dense_noise=False)
    shards = partition_features(prob.view_ptr, 2)
    with _engine(30, 300, 30) as e:
        assert e.exchange_split_rule(prob, shards)["split"]
        e.set_rem_direct_rows(256)                      # the cap the rule compares the batch's remainder rows with
        try:
            assert not e.exchange_split_rule(prob, shards)["split"]
            _root_block_merge(e, prob, shards, ref)
        finally:
            e.set_rem_direct_rows(-1)


def test_root_block_merge_after_a_split_merge():
    """The same engine merges split records, then root blocks of a batch the rule refuses: the second merge has ONE source of
    rows and its own status words (nothing of the split merge's remainder rows or early update may leak into it)."""
    from msckf_amd.shard import partition_features
    prob = synth.make_problem(30, 600, 30, seed=83, variable_tracks=True, min_track=2)
    ref = oracle.update(prob, dense_noise=False)
    shards = partition_features(prob.view_ptr, 4)
    with _engine(30, 600, 30) as e:
        _split_merge(e, prob, shards, ref)
        e.set_rem_direct_rows(256)
        try:
            assert not e.exchange_split_rule(prob, shards)["split"]
            _root_block_merge(e, prob, shards, ref)
        finally:
            e.set_rem_direct_rows(-1)
        _split_merge(e, prob, shards, ref)


def test_a_failed_early_update_reaches_the_shared_result():
    """MSCKF_DEBUG_FAKE_TIMEOUT=1: the merge's first early update on the remainder rows reads as timed out (status word 1 =
    2, a software fake).  Every rank's `shared_result()` must report an error, never status 0; the next merge is clean."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import msckf_amd
from msckf_amd import synth, _ffi
from msckf_amd.shard import partition_features
from oracle import msckf_oracle as oracle
import test_gpu_shard_split as t
prob = synth.make_problem(30, 600, 30, seed=83, variable_tracks=True, min_track=2)
ref = oracle.update(prob, dense_noise=False)
with t._engine(30, 600, 30) as e:
    try:
        t._split_merge(e, prob, partition_features(prob.view_ptr, 4), ref, calls=1)
        print("FAKE_MISSED")
    except _ffi.EngineError as err:
        print("FAKE_SEEN", err.code)
    t._split_merge(e, prob, partition_features(prob.view_ptr, 4), ref)
    print("CLEAN_AFTER")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, MSCKF_DEBUG_FAKE_TIMEOUT="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    from msckf_amd import _ffi
    assert "FAKE_SEEN %d" % _ffi.ERR_HIP in out.stdout and "CLEAN_AFTER" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]



_RCCL_SPLIT = r"""
import os, sys, tempfile
sys.path.insert(0, %(root)r)
import numpy as np
import msckf_amd
from msckf_amd import synth
from msckf_amd.api import UpdateEngine
from msckf_amd.shard import RcclShardedUpdate, exchange_unique_id, partition_features
from oracle import msckf_oracle as oracle
rank, world, idp = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
assert "torch" not in sys.modules

def check(drv, prob, split):
    ref = oracle.update(prob, dense_noise=False)
    drv.load(prob)
    assert drv.split == split
    for _ in range(2):
        drv.step()
    status, dx, P, acc, n_rej = drv.result()
    e_dx = np.linalg.norm(dx - ref["dx"]) / np.linalg.norm(ref["dx"])
    e_P = np.linalg.norm(P - ref["P_new"]) / np.linalg.norm(ref["P_new"])
    assert status == ref["status"] == 0 and e_dx < 1e-8 and e_P < 1e-8, (status, e_dx, e_P)
    assert np.array_equal(acc, ref["accepted"]) and n_rej == prob.F - int(ref["accepted"].sum())

frame = synth.make_problem(30, 300, 30, seed=81, variable_tracks=True, min_track=2, outlier_fraction=0.1, outlier_px=400.0)
unordered = synth.make_problem(24, 60, 24, seed=90, variable_tracks=True, min_track=12)
uv, sl = unordered.obs_uv.copy(), unordered.obs_slot.copy()
for j in range(0, unordered.F, 2):
    a, b = int(unordered.view_ptr[j]), int(unordered.view_ptr[j + 1])
    uv[a:b] = uv[a:b][::-1].copy(); sl[a:b] = sl[a:b][::-1].copy()
unordered.obs_uv, unordered.obs_slot = uv, sl
with UpdateEngine(max_clones=30, max_features=300, max_track=30, device=rank) as e:
    uid = exchange_unique_id(e, rank, world, idp)
    drv = RcclShardedUpdate(e, rank, world, uid, id_path=idp)
    # split records, then on the SAME engine batches the rule refuses (root blocks): nothing of the split merge may leak
    check(drv, frame, True)
    check(drv, unordered, False)
    check(drv, frame, True)
    e.set_rem_direct_rows(256)                       # the frame over the remainder-row cap: root blocks
    check(drv, frame, False)
    e.set_rem_direct_rows(-1)
    check(drv, frame, True)
    drv.close()
print("RCCL_SPLIT_OK", rank, flush=True)
"""


def _rccl_split_run(world, td):
    idp = os.path.join(td, "id")
    env = dict(os.environ, MSCKF_RUN_TAG="shard-split-%d-%d" % (os.getpid(), world))
    procs = [subprocess.Popen([sys.executable, "-c", _RCCL_SPLIT % {"root": ROOT}, str(r), str(world), idp], cwd=ROOT, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        outs.append(o)
    for r, o in enumerate(outs):
        assert "RCCL_SPLIT_OK %d" % r in o, "rank %d:\n%s" % (r, o[-3000:])


def test_rccl_driver_split_records_then_root_blocks(tmp_path):
    """`RcclShardedUpdate` at world 1 (real RCCL collectives, no PyTorch in the process): the frame batch as split records, then
    batches the rule refuses (views out of slot order; the remainder-row cap) as root blocks on the same engine, and back."""
    _rccl_split_run(1, str(tmp_path))


def test_rccl_world2_on_the_frame(tmp_path):
    """Two RCCL ranks, one GPU each (RCCL ranks never share a GPU): split records gathered across ranks."""
    from msckf_amd import _ffi
    if _ffi.load().msckf_device_count() < 2:
        pytest.skip("needs two GPUs")
    _rccl_split_run(2, str(tmp_path))
