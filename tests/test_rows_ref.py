"""The yardstick of the direct measurement rows (tests/rows_ref.py), held to the conditions a tolerance on its cases rests on.
CPU only: nothing of the engine runs here, and the file passes with or without msckf_run_rows.

For every case of the table
  * the exact fp64 forms of the update (the literal MSCKF.py:604-614 algebra, the engine's Cholesky / W form and, for a
    diagonal R, m one-row Joseph updates) agree to 1e-12 in all of filter_prior.metrics: the GPU tests' 1e-8 then has
    four decades of room that belong to the kernels, not to the case;
  * the update removes at least 1e-5 of |P| (no no-information update: the update-term measure would have no floor);
  * a gated case sits on the side of its critical value it is meant to be on, |gamma - crit| / crit >= 1e-6.
Measured here (worst over the table): spread 1.7e-14 (imu_32_N30, scaled_P) in the first four measures, 3.9e-13 in the
update term (pos_N3, whose update removes 1.8e-4 of |P|); smallest update pos_N3, 1.8e-4.
"""
import numpy as np
import pytest

import filter_prior as fp
import rows_ref as rr

NAMES = list(rr.CASES)


def test_the_table_covers_the_shapes():
    cs = rr.CASES.values()
    assert {c.N for c in cs} == {0, 1, 3, 30, 221}
    assert [c.name for c in cs if c.N == 221] == ["dense_32_N221", "zupt_N221"]
    for kind in ("imu", "dense"):
        for N in rr.N_VALUES:
            assert {c.m for c in cs if c.kind == kind and c.N == N and c.gate is None} == {1, 3, 6, 15, 16, 17, 32}
    assert {c.gate for c in cs} == {None, "above", "below", "table"}
    assert not rr.SEED_SKIPS and not rr.NOISE_FACTOR        # every case stands at k = 0 with the stated noise


def test_the_literal_form_is_the_reference_algebra():
    """`update` on a camera-shaped measurement (T_H = [0 | T], R = sigma^2 I) is the oracle's K6-K7: the same lines of
    MSCKF.py, reached from the other side."""
    rng = np.random.default_rng(5)
    P = np.array(fp.filter_prior(3)[0])
    d = P.shape[0]
    T = np.zeros((6, d))
    T[:, 15:] = rng.standard_normal((6, d - 15))
    r, sigma = rng.standard_normal(6), 0.7
    got = rr.update(P, T, r, sigma ** 2 * np.eye(6))
    S = T @ P @ T.T + sigma ** 2 * np.eye(6)
    K = P @ T.T @ np.linalg.inv(S)
    A = np.eye(d) - K @ T
    Pn = A @ P @ A.T + sigma ** 2 * K @ K.T
    from conftest import rel_err
    assert np.array_equal(got["dx"], K @ r)
    assert rel_err(got["P_new"], (Pn + Pn.T) / 2) < 1e-14           # (K (sigma^2 I) K^T against sigma^2 K K^T: roundings only)


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    case = rr.CASES[name]
    (P, H, r, R), crit, ref = rr.problem(name)
    d = 15 + 6 * case.N
    assert P.shape == (d, d) and H.shape[0] == case.m == r.size and R.shape == (case.m, case.m) and H.shape[1] <= d
    assert np.array_equal(R, R.T)
    sp = rr.spread(name)
    rm = rr.removed(name)
    print(f"ROWSREF {name} " + " ".join(f"{x:.2e}" for x in sp) + f" removed {rm:.2e}")
    assert max(sp) <= rr.SPREAD_TOL, sp
    assert rm >= rr.MIN_UPDATE, rm
    if case.gate is not None:
        free = rr.update(P, H, r, R)
        assert abs(free["gamma"] - crit) / crit >= 1e-6
        assert ref["applied"] == (case.gate != "below")
        if not ref["applied"]:
            assert not ref["dx"].any() and np.array_equal(ref["P_new"], P) and ref["status"] == 1


def test_a_nan_residual_is_a_rejection():
    (P, H, r, R), _, _ = rr.problem("imu_6_N30")
    bad = np.array(r)
    bad[2] = np.nan
    for crit in (np.inf, 12.0):
        ref = rr.update(P, H, bad, R, crit)
        assert not ref["applied"] and ref["status"] == 1 and np.array_equal(ref["P_new"], P)
