"""K1-K4 (csrc/k_feature.h) on camera geometries other than the synthetic corridor: every case of tests/geometry_cases.py through the
one-shot `msckf_update` and through load / run / result, against the oracle.

What the corridor pins and these cases do not: the pivot order of K2's column-pivoted QR (all six orders in each of the forms
<24>, <32>, <64>, <64, true[, 4]>, in the one-level loop and in the split's level 2), the rank decision (whole windows of exact
rank-2 tracks: standing still, rotation about one point -- the rank-2 exit of every form, `n_wide_rows = ncarry - 2` in the
split), the split's unpivoted level 1 on a view group of rank 2 inside a track of rank 3 (a stop in the middle, exact and 1e-9 /
1e-6 apart), and K1's signs and scales (pz < 0, rho down to 1e-4, base off every clone, rotated gravity and world axes, two K).

The cases were conditioned on the CPU (tests/test_geometry_cases.py): two exact fp64 algorithms agree to 1e-10 on every one of
them, every rank decision lies a factor 4 from its threshold, no gate verdict within 1e-6 of the threshold.  Asserted here, for
every case, as everywhere else in the suite: the accepted mask the oracle's; `msckf_debug_gate`'s row count 2M - rank per track;
gamma at rtol 1e-9; `msckf_debug_compressed` T^T T = H^T H and T^T r_n = H^T r at 1e-8; dx and P+ at 1e-8 in the five measures of
`filter_prior.metrics`.  Each check prints `GEOMETRYGPU <case> <path> ...`; the worst per family are in DESIGN.md section 5."""
import os
import subprocess
import sys

import numpy as np
import pytest

import failing_batches as fb
import filter_prior as fp
import geometry_cases as gc
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-8
TOL_F32 = (1e-4, 1e-5)                          # the f32 mode's flat pair (tests/test_gpu_f32.py)
GAMMA_TOL = dict(rtol=1e-9, atol=1e-12)         # tests/test_gpu_gate_not_spd.py

SPLIT_CASES = [n for n, c in gc.CASES.items() if c.form == "split"]
BAND_CASES = [n for n, c in gc.CASES.items() if c.form in ("k24", "k32", "k64")]
SUBSET = sorted({c.family: n for n, c in gc.CASES.items() if c.form == "split"}.values())      # one case per family


def engine(**kw):
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=34, max_features=256, max_track=31)
    args.update(kw)
    return UpdateEngine(**args)


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


def check_result(name, what, res, prob, ref, tol=(TOL, TOL)):
    m = fp.metrics(res.dx, res.P_new, ref, prob.P)
    print(f"GEOMETRYGPU {name} {what} " + " ".join(f"{x:.2e}" for x in m), flush=True)
    assert res.status == ref["status"] == 0, (name, what)
    assert np.array_equal(res.accepted, ref["accepted"]), (name, what)
    assert res.stats["not_spd"] == 0 and res.stats["n_accepted"] == int(ref["accepted"].sum()), (name, what, res.stats)
    assert np.array_equal(res.P_new, res.P_new.T), (name, what)
    e_dx, e_P, s_dx, s_P, u_P = m
    assert e_dx < tol[0] and e_P < tol[1], (name, what, e_dx, e_P)
    if tol == (TOL, TOL):
        assert s_dx < TOL and s_P < TOL and u_P < TOL, (name, what, s_dx, s_P, u_P)


def check_debug(e, name, what, prob, ref, split):
    """The rank decision per track, gamma, the compressed system, and what the blocks of split tracks inherited."""
    case = gc.CASES[name]
    M = np.diff(prob.view_ptr)
    gam, q = e.debug_gate()
    assert np.array_equal(q, 2 * M - (2 if case.exact_rank2 else 3)), (name, what, q, M)
    err = float(np.max(np.abs(gam - ref["gamma"]) / np.abs(ref["gamma"])))
    T, rn = e.debug_compressed()
    H, r = ref["H_X"][:, 15:], ref["r_o"]
    e_T, e_r = rel_err(T.T @ T, H.T @ H), rel_err(T.T @ rn, H.T @ r)
    print(f"GEOMETRYGPU {name} {what} gamma {err:.2e} TtT {e_T:.2e} Ttr {e_r:.2e}", flush=True)
    np.testing.assert_allclose(gam, ref["gamma"], **GAMMA_TOL)
    assert e_T < TOL and e_r < TOL, (name, what, e_T, e_r)
    codes, block_codes, block_track = e.gate_codes()
    assert np.array_equal(codes, ref["accepted"]), (name, what)
    long = fb.long_tracks(prob) if split else np.zeros(prob.F, dtype=bool)
    s = e.debug_split()
    assert s["long_tracks"] == int(long.sum()), (name, what, s)
    if long.any():
        assert len(block_codes) == s["entries"] - prob.F > 0
        assert set(block_track.tolist()) == set(np.nonzero(long)[0].tolist())
        assert np.array_equal(block_codes, codes[block_track]), (name, what)        # a block carries its track's byte
    else:
        assert len(block_codes) == 0


def run_case(e, name, direct_rows=-1, what="", split=True, bit_equal=False):
    """One case through the one-shot call and through load / run / result on the resident state."""
    prob, ref = gc.problem(name)
    e.set_rem_direct_rows(direct_rows)
    try:
        res = e.update_problem(prob)
        check_result(name, what + "one-shot", res, prob, ref)
        check_debug(e, name, what + "one-shot", prob, ref, split)
        assert res.stats["stacked_rows"] == ref["H_X"].shape[0]
        if split and gc.CASES[name].form == "split":
            s = e.debug_split()
            assert s["long_tracks"] > 0 and s["narrow_blocks"] > 0, s         # at least one long track really split
            assert s["remainder_mode"] == (1 if direct_rows < 0 else 2), s
        e.load(prob)
        e.run()
        res2 = e.result()
        check_result(name, what + "resident", res2, prob, ref)
        check_debug(e, name, what + "resident", prob, ref, split)
        if bit_equal:
            assert np.array_equal(res2.dx, res.dx) and np.array_equal(res2.P_new, res.P_new), name
    finally:
        e.set_rem_direct_rows(-1)


# ---- every case, every form --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BAND_CASES)
def test_unsplit_forms(eng, name):
    """k_feature<24>, <32> (tracks of 11 - 15 views, most of the batch: 90-column tiles) and <64> (views in descending slot
    order: a long track keeps one block)."""
    run_case(eng, name)
    assert eng.debug_split()["long_tracks"] == 0


@pytest.mark.parametrize("direct_rows", [-1, 0], ids=["rows", "tree"])
@pytest.mark.parametrize("name", SPLIT_CASES)
def test_split_form(eng, name, direct_rows):
    """k_feature<64, true, 4>: remainder rows as they are and through their own tree."""
    run_case(eng, name, direct_rows)


def test_tree_plan():
    """plan="tree": every track through the merge tree's leaves (k_fold_g: N = 34, leaves of up to 1024 rows)."""
    name = "rotated_tree"
    with engine(max_features=64, plan="tree", leaf_rows=1024) as e:
        run_case(e, name, what="tree plan ", split=False)
        s = e.debug_split()
        assert s["band_plan"] == 0 and s["long_tracks"] == 0, s


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import msckf_amd
import test_gpu_geometry as t
with t.engine() as e:
    for name in t.SPLIT_CASES:
        t.run_case(e, name, -1, what="one wavefront ")
        t.run_case(e, name, 0, what="one wavefront, tree ")
print("FORM_OK")
"""


def test_split_form_with_one_wavefront_per_track():
    """k_feature<64, true>: MSCKF_SPLIT_MW_MAX is read once per process."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MSCKF_SPLIT_MW_MAX="0"), cwd=ROOT)
    print(out.stdout[-20000:])
    assert out.returncode == 0 and "FORM_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- one case per family: the other consumers -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SUBSET)
def test_one_shot_equals_resident_bit_for_bit(eng, name):
    run_case(eng, name, bit_equal=True, what="bitwise ")


@pytest.fixture(scope="module")
def eng_f32():
    e = engine(dtype="f32")
    yield e
    e.close()


@pytest.mark.parametrize("name", SUBSET)
def test_f32_mode(eng_f32, name):
    prob, ref = gc.problem(name)
    res = eng_f32.update_problem(prob)
    check_result(name, "f32", res, prob, ref, TOL_F32)
    M = np.diff(prob.view_ptr)
    assert np.array_equal(eng_f32.debug_gate()[1], 2 * M - (2 if gc.CASES[name].exact_rank2 else 3))


@pytest.fixture(scope="module")
def eng_shards():
    e = engine()
    yield e
    e.close()


@pytest.mark.parametrize("name", SUBSET)
def test_two_logical_shards(eng_shards, name):
    """The calls of `RcclShardedUpdate.load / step / result` with two logical shards on one engine (split records)."""
    from msckf_amd.shard import partition_features
    from test_gpu_shard_split import _split_merge
    prob, ref = gc.problem(name)
    res = _split_merge(eng_shards, prob, partition_features(prob.view_ptr, 2), ref)
    m = fp.metrics(res.dx, res.P_new, ref, prob.P)
    print(f"GEOMETRYGPU {name} two shards " + " ".join(f"{x:.2e}" for x in m), flush=True)
    assert max(m) < TOL, (name, m)
