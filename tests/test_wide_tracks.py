"""Tracks of more than 31 views, the CPU side: the oracle against the reference-pinned fixture
`golden/wide/edge_wide_tracks.npz` (reference `MSCKF.py:570-614`; written by `golden/gen_wide_golden.py`), the gate margins
of every batch tests/test_gpu_wide_tracks.py holds against a reference, and the limit the Python layer names."""
import numpy as np

import wide_cases as wc
from conftest import rel_err
from oracle import msckf_oracle as oracle


def test_oracle_against_the_wide_fixture():
    prob, z = wc.fixture()
    v = wc.views(prob)
    assert prob.N == 40 and prob.F == 24 and v.min() >= 20 and v.max() <= 40 and int(wc.wide(prob).sum()) == 12
    acc = z["accepted"].astype(bool)
    assert int(acc.sum()) == 16 and (wc.wide(prob) & acc).any() and (wc.wide(prob) & ~acc).any()
    assert set(z["versions"].shape) == {3}
    ref = oracle.update(prob, dense_noise=False)
    assert ref["status"] == int(z["status"]) == 0
    assert np.array_equal(ref["accepted"], z["accepted"])
    e_dx, e_P = rel_err(ref["dx"], z["dx"]), rel_err(ref["P_new"], z["P_new"])
    print(f"oracle against the fixture: dx {e_dx:.2e}, P+ {e_P:.2e}")
    assert e_dx < 1e-9 and e_P < 1e-9, (e_dx, e_P)
    np.testing.assert_allclose(ref["gamma"], z["gamma"], rtol=1e-8, atol=1e-12)
    assert abs(wc.margin(z) - 0.31) < 0.01                     # the smallest |gamma - crit| / crit of the batch


def test_no_gpu_case_sits_on_a_gate_threshold():
    """A gate decision within rounding of its threshold is no parity case: every batch of the GPU file keeps its smallest
    |gamma - crit| / crit at or above 1e-3 on the oracle (or the restatement with per-view noise)."""
    margins = wc.gpu_case_margins()
    print({k: round(v, 4) for k, v in margins.items()})
    assert set(wc.SYNTH) <= set(margins)
    for name, m in margins.items():
        assert m >= wc.MIN_MARGIN, (name, m)


def test_the_cases_hold_what_they_are_for():
    first, cap, mixed = (wc.views(wc.synth_case(n)[0]) for n in ("first", "cap", "mixed"))
    assert {32, 33, 34} <= set(first.tolist()) and first.min() >= 32
    assert 2 * first.sum() - 3 * len(first) > 15 + 6 * 34                      # more rows than d: the QR branch
    assert cap.tolist() == [64, 64, 64] and 2 * cap.sum() - 9 < 15 + 6 * 64   # the no-QR branch at the widest gate matrix
    assert int((mixed >= wc.WIDE_FROM).sum()) == 4 and mixed.min() == 2
    prob, ref, rows = wc.rank2_case()
    assert wc.wide(prob).all() and np.array_equal(rows, 2 * wc.views(prob) - 2)        # rank 2 on every track
    prob, _ = wc.reversed_case()
    assert wc.wide(prob).all() and all(np.all(np.diff(prob.obs_slot[a:b]) < 0) for a, b in zip(prob.view_ptr[:-1], prob.view_ptr[1:]))
    prob, bad, good, ref = wc.not_spd_case()
    assert wc.wide(prob).all() and bad.any() and len(good) > 0 and ref["status"] == 0
    assert wc.not_spd_case(16)[1].all()                                               # every track sees clone 16


def test_python_names_the_wide_limit():
    from msckf_amd import _ffi
    assert _ffi.MAX_TRACK_WIDE >= 64 and _ffi.MAX_TRACK == 31 and _ffi.MAX_TRACK_ROW == 32
