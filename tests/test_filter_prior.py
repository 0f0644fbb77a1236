"""tests/filter_prior.py on the CPU: what makes its priors, its cases and its metrics fit to hold the engine to.

  1. The generator makes what it claims: the statistics of a covariance that a filter produced, inside the same inequalities as
     the reference's own priors (the `*_B` fixtures), and `ops` is all of what built it.
  2. Every entry of CASES meets its conditions -- these are conditions on the INPUTS, decided here, before any GPU run: the
     oracle's status, both sides of the gate, no verdict at the threshold, and a reference spread (two correct fp64 algorithms
     against each other) four orders below what tests/test_gpu_filter_prior.py asserts.
  3. The three metrics see what `rel_err` does not: defects that pass the Frobenius 1e-8 by orders of magnitude.

Seen (this file's prints, `-s`): in the tests' own docstrings."""
import numpy as np
import pytest

import filter_prior as fp
from conftest import load_golden, rel_err

TOL = 1e-8
SPREAD = 1e-12


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------

def _filter_shaped(P, what):
    lo, hi, off, ratio = fp.statistics(P)
    print(f"{what}: correlation spectrum {lo:.1e} .. {hi:.1f}, largest correlation {off:.6f}, max / min sigma {ratio:.0f}")
    assert np.array_equal(P, P.T)
    assert -1e-12 <= lo <= 1e-9 * hi                         # singular PSD: the newest clone is a function of the IMU state
    assert off >= 0.999
    assert ratio >= 30


@pytest.mark.parametrize("N", [10, 20, 30, 107])
def test_the_generator_makes_a_filter_shaped_prior(N):
    P, cam_R, cam_t, ops, imu = fp.filter_prior(N)
    assert P.shape == (15 + 6 * N,) * 2 and cam_R.shape == (N, 3, 3) and cam_t.shape == (N, 3)
    assert len(ops) == 3 * N and len(imu) == 2 * N
    _filter_shaped(P, f"filter_prior({N})")
    assert np.array_equal(fp.replay(ops, fp.head()["P0"]), P)          # bit for bit: ops is everything that was applied
    again = fp.filter_prior(N)
    assert again[0] is P                                               # memoised
    from msckf_amd import synth
    traj_R, traj_t = synth.clone_poses(N, np.random.default_rng([fp.PRIOR_SEED, 0]))
    assert np.max(np.abs(cam_R - traj_R)) < 1e-15 and np.max(np.abs(cam_t - traj_t)) < 1e-15     # synth.clone_poses' trajectory


@pytest.mark.parametrize("case", ["cfg1_B", "cfg2_B", "edge_long_tracks_B"])
def test_the_references_own_priors_meet_the_same_inequalities(case):
    """What pins the generator to the reference: the fixtures that hold a covariance the reference's filter produced."""
    prob, _ = load_golden(case)
    _filter_shaped(prob.P, case)


@pytest.mark.parametrize("case,N", [("cfg1_B", 10), ("cfg2_B", 20), ("edge_long_tracks_B", 30)])
def test_the_clock_is_the_fixtures(case, N):
    """filter_prior's one free scale, the time between two frames: at 0.1 s the spread of sigma is the fixture's of the same
    width to 2.5 % (103 / 209 / 454 against 102 / 205 / 446), held here to 10 %.  Past 30 clones the window keeps the 3 s span."""
    prob, _ = load_golden(case)
    assert prob.N == N and fp.frame_dt(N) == fp.FRAME_DT
    ours, theirs = fp.statistics(fp.filter_prior(N)[0])[3], fp.statistics(prob.P)[3]
    print(f"{case}: max / min sigma {theirs:.0f}, filter_prior({N}) {ours:.0f}")
    assert 0.9 < ours / theirs < 1.1
    assert fp.frame_dt(31) * 31 == pytest.approx(fp.SPAN) and fp.frame_dt(221) * 221 == pytest.approx(fp.SPAN)


def test_the_covariances_kept_on_the_way_are_the_replayed_prefixes():
    P, _, _, ops, _ = fp.filter_prior(54)
    assert fp.on_the_way(54, 54) is P
    for n in (1, 11, 53):
        assert np.array_equal(fp.replay(ops[:3 * n], fp.head()["P0"]), fp.on_the_way(54, n))


# ---- 2. the conditions on every case ------------------------------------------------------------------------------------------

def _meets(name, k):
    prob, ref = fp.problem(name, k)
    case = fp.CASES[name]
    assert (prob.N, prob.F) == (case.N, case.F)
    n_acc = int(ref["accepted"].sum())
    if ref["status"] != 0 or not (name in fp.ONE_SIDED or 0 < n_acc < prob.F):
        return False, f"status {ref['status']}, accepted {n_acc} / {prob.F}"
    margin = fp.gate_margin(ref)
    if margin < 1e-6:
        return False, f"gate margin {margin:.1e}"
    s = fp.spread(prob, ref)
    text = (f"accepted {n_acc} / {prob.F}, gate margin {margin:.1e}, reference spread scaled dx {s[0]:.1e} scaled P {s[1]:.1e} "
            f"update term {s[2]:.1e} Frobenius dx {s[3]:.1e}")
    return max(s) <= SPREAD, text


@pytest.mark.parametrize("name", list(fp.CASES))
def test_every_case_meets_its_conditions(name):
    """The recorded seed meets every condition and every seed skipped on the way to it does not.  Seen: every case
    takes its base seed; reference spread at most 3.5e-15 (scaled dx, stream_82), 3.4e-13 (scaled P, long_31), 3.4e-13 (update
    term, chain_221_F2), 3.2e-13 (Frobenius dx, forms_31); gate margins from 2.6e-2 up."""
    if name in fp.NO_ROWS:
        prob, ref = fp.problem(name)
        assert ref["status"] == 1 and not ref["accepted"].any() and np.array_equal(ref["P_new"], prob.P)
        return
    skipped = fp.SEED_SKIPS.get(name, (0,))[0]
    ok, text = _meets(name, None)
    print(f"{name} (seed {fp.case_seed(fp.CASES[name])}, {skipped} skipped): {text}")
    assert ok, text
    for k in range(skipped):
        assert not _meets(name, k)[0]


# ---- 3. what rel_err cannot see on a filter-shaped prior ------------------------------------------------------------------------
#
# How blind the Frobenius norm is depends on how much of P the update removes.  Two priors, both filter-shaped:
#   early    frames 10 ms apart (two of seq_short's 5 ms samples): the filter 0.3 - 0.6 s after its start.  The update removes
#            0.1 - 0.2 % of |P| and hardly touches the biases.  This is where the blind spot is widest, and where it was first measured.
#   default  filter_prior's own clock (0.1 s, 3 s span): the priors of CASES.  The update removes more than half of |P|.
EARLY = 0.01
BIAS, COLS, DX = "gyro-bias block left at the prior", "last 16 columns of the update term off by 1e-6", "dx[3:6] off by 1e-4"
# rel_err < 1e-8 asserted: on the early prior the bias block at both widths and the 16 columns at N = 30 (seen: 7.1e-11 / 5.0e-11
# and 3.7e-10; the columns at N = 60 are at 9.7e-10, printed); on the default prior the bias block at N = 60 (4.1e-9, with the
# block's variance 1.2 % off; at N = 30 it is 1.3e-8 with the variance 2.1 % off)
BLIND = {("early", BIAS, 30), ("early", BIAS, 60), ("early", COLS, 30), ("default", BIAS, 60)}
# a new metric > 1e-8 asserted: everywhere but dx[3:6] on the early prior, where the whole bias correction is 1.5e-5 (N = 30) and
# 1.9e-4 (N = 60) of the bias sigma -- 1e-4 of that is 1.5e-9 / 1.9e-8 sigma, and a measure in covariance units says so
SEEN = {(prior, what, N) for prior in ("early", "default") for what in (BIAS, COLS, DX) for N in (30, 60)} - {("early", DX, 30)}


def _defect_problem(N, prior):
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    P, cam_R, cam_t, _, _ = fp.filter_prior(N, frame=EARLY if prior == "early" else None)
    prob = synth.make_problem(N, 200, 10, seed=23000 + N, variable_tracks=True, outlier_fraction=0.15, outlier_px=300.0,
                              P=np.array(P), poses=(cam_R, cam_t))
    return prob, oracle.update(prob, dense_noise=False)


@pytest.mark.parametrize("prior", ["early", "default"])
@pytest.mark.parametrize("N", [30, 60])
def test_the_metrics_see_what_rel_err_does_not(N, prior):
    """Three defects built from the oracle's own result (N = 30 / 60, F = 200, tracks of 2 - 10 views, 15 % outliers).  Seen, as
    rel_err | scaled dx or P | update term:
      early    bias block never updated 7.1e-11 / 5.0e-11 | 3.0e-6 / 5.2e-6 | 8.0e-8 / 2.3e-8; 16 columns of the subtracted term
               1e-6 off 3.7e-10 / 9.7e-10 | 5.4e-9 / 9.0e-9 | 4.1e-7 / 4.4e-7; dx[3:6] 1e-4 off 2.7e-8 / 2.0e-8 | 1.5e-9 / 1.9e-8
      default  bias block 1.3e-8 / 4.1e-9 | 2.1e-2 / 1.2e-2 | 1.3e-8 / 5.2e-9; 16 columns 7.3e-7 / 4.7e-7 | 1.5e-5 / 3.9e-6 |
               7.4e-7 / 6.0e-7; dx[3:6] 2.3e-8 / 6.4e-9 | 1.3e-7 / 1.7e-7
    So a gyro-bias block that the update never touched passes the Frobenius 1e-8 by two orders on the early prior, and on the
    default one a bias variance 1.2 % off still passes it; scaled_P sees both by 2 - 6 orders.  The columns need the update term
    on the early prior (scaled_P alone is below 1e-8 there): the metrics are asserted together."""
    prob, ref = _defect_problem(N, prior)
    assert ref["status"] == 0
    P, Pn, dx, d = prob.P, ref["P_new"], ref["dx"], prob.d
    bias = Pn.copy()
    bias[3:6, 3:6] = P[3:6, 3:6]
    term = P - Pn
    term[:, d - 16:] *= 1 + 1e-6
    term[d - 16:, :] = term[:, d - 16:].T
    cols = P - term
    dxb = dx.copy()
    dxb[3:6] *= 1 + 1e-4
    s = fp.spread(prob, ref)
    print(f"N = {N} {prior}: |P - P+| / |P| {rel_err(Pn, P):.1e}, reference spread {s[0]:.1e} {s[1]:.1e} {s[2]:.1e} {s[3]:.1e}")
    assert max(s) <= SPREAD                                            # the measures are well-posed on these priors too
    for what, got_dx, got_P in ((BIAS, dx, bias), (COLS, dx, cols), (DX, dxb, Pn)):
        e_dx, e_P, s_dx, s_P, u_P = fp.metrics(got_dx, got_P, ref, P)
        print(f"N = {N} {prior}: {what}: rel_err dx {e_dx:.1e} P+ {e_P:.1e} | scaled dx {s_dx:.1e} scaled P {s_P:.1e} update term {u_P:.1e}")
        if (prior, what, N) in BLIND:
            assert e_dx < TOL and e_P < TOL, what                      # the blind spot, stated in a test
        if (prior, what, N) in SEEN:
            assert max(s_dx, s_P, u_P) > TOL, what
    # ... and on the oracle's own result the new metrics are zero
    assert fp.metrics(dx, Pn, ref, P) == (0.0,) * 5


def test_the_metrics_on_hand_made_arrays():
    ref = np.array([[4.0, 1.0], [1.0, 1e-6]])
    got = ref + np.array([[0.0, 0.0], [0.0, 1e-9]])
    assert fp.scaled_P(got, ref) == pytest.approx(1e-3) and rel_err(got, ref) < 1e-9
    assert fp.scaled_dx([1.0, 2e-3], [1.0, 1e-3], ref) == pytest.approx(1.0)
    prior = ref + np.eye(2)
    assert fp.update_term(got, ref, prior) == pytest.approx(1e-9 / np.linalg.norm(prior - ref))
