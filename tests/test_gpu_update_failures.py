"""Every launch path of K6-K7 (the sequential 16-row block update) reports a failed pivot: a batch whose gates all pass but
whose joint innovation covariance is indefinite (failing_batches.py; test_failing_batches.py pins what each one means) must
come back as MSCKF_ERR_NOT_SPD through every entry point, with dx = 0 and P_out the prior bit for bit, commit_covariance
refusing it and the resident prior untouched -- on a fresh engine (zeros in P_out) and on a warm one (the last good P+ there).
The next good batch on the same engine matches the oracle.

Paths: the early launch on >= 20 dense remainder row blocks (status word 1, k_gain_dense; k_gain_stream at N = 40), the
remainder rows inside the root's launch, the root's update behind a good early launch, the remainder tree's second update
(whole tree: launch_gain_chain; cut: launch_gain_chain_dense; status word 1), the tree plan, dtype f32, short tracks alone.
The environment switches are read once per process: one child process per setting."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import failing_batches as fb
from conftest import ROOT, rel_err
from msckf_amd import synth
from msckf_amd import _ffi
from msckf_amd._ffi import EngineError, ERR_NOT_SPD
from oracle import msckf_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 1e-8
TOL_F32 = (1e-4, 1e-5)          # the f32 mode's tolerance on dx, P+ (test_gpu_f32.py)
ENTRIES = ("update", "run", "select", "commit")

# case: (failing batch, engine keywords, MSCKF_REM_CUT_ROWS or None, remainder rows taken as they are (-1) or by a tree (0),
#        the remainder mode msckf_debug_split must report: 0 nothing split, 1 dense rows, 2 a tree; None: not checked)
CASES = {
    "short": ("spd_p", {}, None, -1, 0),
    "early": ("early", {}, None, -1, 1),
    "root": ("root", {}, None, -1, 1),
    "inroot": ("inroot", {}, None, -1, 1),
    "chain": ("hole", {}, "0", 0, 2),
    "chain_cut": ("hole", {}, "1000", 0, 2),
    "tree": ("early", {"plan": "tree"}, None, -1, None),
    "f32_short": ("spd_p", {"dtype": "f32"}, None, -1, 0),
    "f32_split": ("early", {"dtype": "f32"}, None, -1, 1),
    "wide": ("wide", {}, None, -1, 1),
}
# (MSCKF_GAIN_STREAM=0: round 3's K6-K7 launches, which take no split tracks)
SPLIT_ON = os.environ.get("MSCKF_GAIN_STREAM", "1") != "0"

_PROBS = {}


def _batch(name):
    if name not in _PROBS:
        _PROBS[name] = fb.spd_p_problem() if name == "spd_p" else fb.twin(name)
    return _PROBS[name]


def _good_batch(N):
    """A frame of the reference's shape (tracks ~ U[2, 30], so >= 20 remainder row blocks: the early launch runs) in the same window."""
    key = ("good", N)
    if key not in _PROBS:
        _PROBS[key] = synth.make_problem(N, 300, 30, seed=N, variable_tracks=True, min_track=2)
    return _PROBS[key]


_REFS = {}


def _ref(prob, key, select):
    k = (key, select)
    if k not in _REFS:
        if select:
            tracks = fb.select_tracks(prob)
            valid, sub = fb.selected(prob, tracks)
            _REFS[k] = (tracks, valid, oracle.update(sub, dense_noise=False))
        else:
            _REFS[k] = (None, None, oracle.update(prob, dense_noise=False))
    return _REFS[k]


def _raw_result(eng):
    """msckf_get_result without the wrapper's raise: (code, dx, P_out), the arrays filled with NaN beforehand."""
    d = 15 + 6 * eng._N
    dx, P = np.full(d, np.nan), np.full((d, d), np.nan)
    acc = np.zeros(max(eng._F, 1), dtype=np.uint8)
    st = _ffi.Stats()
    rc = eng._lib.msckf_get_result(eng._h, _ffi.dptr(dx), _ffi.dptr(P), _ffi.uptr(acc), C.byref(st))
    return rc, dx, P


def _load_run(eng, prob, entry, tracks):
    eng.load(prob)
    if entry == "select":
        eng.set_tracks(tracks)
        eng.run_select(fb.SELECT, prob.K)
    eng.run()


def expect_failure(eng, prob, entry):
    P0 = prob.P
    if entry == "update":
        with pytest.raises(EngineError) as ei:
            eng.update_problem(prob)
        assert ei.value.code == ERR_NOT_SPD, ei.value
    else:
        _load_run(eng, prob, entry, fb.select_tracks(prob) if entry == "select" else None)
        if entry != "commit":
            rc, dx, P = _raw_result(eng)
            assert rc == ERR_NOT_SPD, rc
            assert not dx.any() and np.array_equal(P, P0)
    assert eng._lib.msckf_commit_covariance(eng._h) == ERR_NOT_SPD
    assert np.array_equal(eng.covariance(), P0)                 # the resident prior is untouched


def expect_good(eng, prob, entry, key, tol=(TOL, TOL)):
    tracks, valid, ref = _ref(prob, key, entry == "select")
    assert ref["status"] == 0
    if entry == "update":
        res = eng.update_problem(prob)
    else:
        _load_run(eng, prob, entry, tracks)
        if entry == "commit":
            assert eng.commit_covariance() == 0
            assert rel_err(eng.covariance(), ref["P_new"]) < tol[1]
            return
        res = eng.result()
    assert res.status == 0
    acc = res.accepted if valid is None else res.accepted[valid]
    assert np.array_equal(acc, ref["accepted"])
    assert rel_err(res.dx, ref["dx"]) < tol[0] and rel_err(res.P_new, ref["P_new"]) < tol[1]
    assert eng.commit_covariance() == 0
    assert np.array_equal(eng.covariance(), res.P_new)


def run_case(case, entry, warm):
    """One cell of the matrix on an engine of its own: [good batch], failing batch, good batch."""
    from msckf_amd.api import UpdateEngine
    bad_name, kw, cut, rem_rows, mode = CASES[case]
    bad = _batch(bad_name)
    good = _good_batch(bad.N)
    tol = TOL_F32 if kw.get("dtype") == "f32" else (TOL, TOL)
    old_cut = os.environ.pop("MSCKF_REM_CUT_ROWS", None)
    if cut is not None:
        os.environ["MSCKF_REM_CUT_ROWS"] = cut                   # (read when a context is created)
    try:
        with UpdateEngine(max_clones=bad.N, max_features=400, max_track=30, **kw) as eng:
            eng.set_rem_direct_rows(rem_rows)
            if warm:
                expect_good(eng, good, entry, ("good", bad.N), tol)
            expect_failure(eng, bad, entry)
            if mode is not None and SPLIT_ON:                   # the batch took the path the case is about
                s = eng.debug_split()
                assert s["remainder_mode"] == mode and s["long_tracks"] == (bad.F if mode else 0), s
                if mode == 1:
                    assert (s["remainder_rows_cap"] + 15) // 16 == fb.remainder_blocks(bad)
            expect_good(eng, good, entry, ("good", bad.N), tol)
    finally:
        os.environ.pop("MSCKF_REM_CUT_ROWS", None)
        if old_cut is not None:
            os.environ["MSCKF_REM_CUT_ROWS"] = old_cut


@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_failed_update_is_reported(case, entry, warm):
    run_case(case, entry, warm)


def run_stale_word(case, entry):
    """A failed update whose status went to word 1 (the early launch or the remainder tree's second update), then a batch of a few
    long tracks (90 remainder rows, 6 blocks: inside the root's launch, nothing writes word 1): status 0 and the oracle's update,
    not the stale word's NOT_SPD."""
    from msckf_amd.api import UpdateEngine
    bad_name, kw, cut, rem_rows, _ = CASES[case]
    bad = _batch(bad_name)
    few = synth.few_long_tracks_problem(30, 400, 10, 10)
    with UpdateEngine(max_clones=bad.N, max_features=400, max_track=30, **kw) as eng:
        eng.set_rem_direct_rows(rem_rows)
        expect_failure(eng, bad, "run")
        eng.set_rem_direct_rows(-1)
        expect_good(eng, few, entry, "few")
        assert eng.debug_split()["remainder_mode"] == 1 and eng.debug_split()["remainder_rows_cap"] == 90


@pytest.mark.parametrize("entry", ["select", "commit"])             # the entries that read word 1 back from the device
@pytest.mark.parametrize("case", ["early", "chain"])
def test_stale_status_word_is_not_read(case, entry):
    run_stale_word(case, entry)


def test_failed_early_update_of_a_sharded_merge():
    """The merge of split records (4 logical shards on one engine) with a real indefinite prior: its early update on the
    collected remainder rows fails, and the shared result every rank reads says so; the next merge is clean."""
    import test_gpu_shard_split as t
    from msckf_amd.shard import partition_features
    bad = _batch("early")
    with t._engine(bad.N, 400, 30) as e:
        with pytest.raises(EngineError) as ei:
            t._split_merge(e, bad, partition_features(bad.view_ptr, 4), _ref(bad, "early", False)[2], calls=1)
        assert ei.value.code == ERR_NOT_SPD
        good = _good_batch(bad.N)
        t._split_merge(e, good, partition_features(good.view_ptr, 4), _ref(good, ("good", bad.N), False)[2])


def test_root_block_merge_behind_a_failed_run():
    """A failed early update leaves status word 1 = 1 on the device; a root-block merge on the same engine (one source of rows,
    nothing of it writes word 1) is then read by msckf_commit_covariance ALONE -- the reader that does its own read-back meets
    the record of a run of another kind -- and, the same sequence again, by msckf_get_result: status 0 and the oracle's update."""
    from msckf_amd.api import UpdateEngine
    bad = _batch("early")
    good = synth.make_problem(30, 64, 6, seed=1)
    ref = oracle.update(good, dense_noise=False)
    assert good.N == 30 and ref["status"] == 0
    with UpdateEngine(max_clones=max(bad.N, good.N), max_features=400, max_track=30) as eng:     # (the failing batch has 34 clones)
        for reader in ("commit", "result"):
            eng.set_rem_direct_rows(-1)
            eng.load(bad)
            eng.run()
            assert _raw_result(eng)[0] == ERR_NOT_SPD
            eng.load(good)
            eng.run_compress()
            blk, n_acc = eng.export_block()
            assert n_acc == int(ref["accepted"].sum())
            eng.merge_gain(blk[None], n_acc)
            if reader == "commit":
                assert eng._lib.msckf_commit_covariance(eng._h) == 0
                e_P = rel_err(eng.covariance(), ref["P_new"])
                print("commit", e_P, flush=True)
                assert e_P < TOL
            else:
                res = eng.result()
                e_dx, e_P = rel_err(res.dx, ref["dx"]), rel_err(res.P_new, ref["P_new"])
                print("result", res.status, e_dx, e_P, flush=True)
                assert res.status == 0 and e_dx < TOL and e_P < TOL


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import msckf_amd
import test_gpu_update_failures as t
for case in %r:
    for entry in t.ENTRIES:
        for warm in (False, True):
            t.run_case(case, entry, warm)
            print("CELL", case, entry, warm, flush=True)
for case in %r:
    t.run_stale_word(case, "commit")
    print("STALE", case, flush=True)
print("MATRIX_OK")
"""


@pytest.mark.parametrize("env,cases,stale", [
    ({"MSCKF_T2_EARLY_MIN": "1"}, ["inroot", "root"], ["early"]),            # every batch with split tracks: the early launch
    ({"MSCKF_T2_EARLY_MIN": "100000"}, ["early", "root"], []),              # never: the remainder rows in the root's launch
    ({"MSCKF_T2_SPLIT_ROOT": "0"}, ["early", "root"], ["early"]),           # the root's sweep and update in one launch behind the early one
    ({"MSCKF_GAIN_DENSE": "0"}, ["early", "chain_cut"], ["early"]),         # the one-block kernel on dense rows
    ({"MSCKF_DIRECT_RESULT": "0"}, ["early", "inroot", "chain"], ["early", "chain"]),   # status | dx | P+ read back from the device
    ({"MSCKF_GAIN_STREAM": "0"}, ["short", "early"], []),                   # round 3's K6-K7 launches (no split)
], ids=["t2_early_min_1", "t2_early_never", "t2_split_root_0", "gain_dense_0", "direct_result_0", "gain_stream_0"])
def test_failed_update_is_reported_under_switch(env, cases, stale):
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), cases, stale)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **env), cwd=ROOT)
    assert "MATRIX_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
