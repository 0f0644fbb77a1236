"""tests/prior_ref.py, the restatement of the update with priors on the tracks' points, against itself and the oracle (CPU).

Its two forms -- three whitened prior rows in front of the null-space projection, and the EKF update with the residual
r - H_f (pbar - p_lin) under the noise sigma^2 I + H_f Sigma_p H_f^T -- are the same update, on every shape of the GPU cases,
with the priors as drawn and linearised at the mean (and under heterogeneous per-view noise on "band").

Figures: gamma as the worst relative difference over the tracks, dx and P+ as norm of the difference over the norm.  Measured
(x86-64, NumPy with OpenBLAS), as drawn / at the mean:
    one_view            gamma 9.2e-15 / 1.3e-15   dx 1.8e-15 / 2.2e-15   P+ 7.2e-17 / 3.4e-17
    one_chunk           gamma 3.8e-16 / 2.0e-13   dx 1.8e-15 / 1.3e-12   P+ 1.7e-16 / 6.0e-13
    band                gamma 2.2e-15 / 9.3e-16   dx 2.1e-15 / 3.8e-15   P+ 2.1e-16 / 2.1e-16
    band, view_sigma    gamma 1.5e-15 / 2.4e-15   dx 1.9e-15 / 2.3e-15   P+ 2.0e-16 / 2.0e-16
    tiles90             gamma 4.1e-15 / 1.3e-15   dx 2.0e-15 / 4.5e-15   P+ 2.0e-16 / 2.1e-16
    thirty              gamma 1.6e-15 / 2.2e-15   dx 2.6e-15 / 1.4e-15   P+ 1.9e-16 / 1.9e-16
    split_beside        gamma 8.7e-16 / 6.8e-16   dx 1.9e-15 / 2.1e-15   P+ 2.4e-16 / 2.6e-16
    split_beside_long   gamma 6.0e-16 / 1.3e-15   dx 1.6e-15 / 2.0e-15   P+ 2.3e-16 / 2.1e-16
(one_chunk at the mean: the track whose mean was moved 10 m is linearised there and passes the gate with residuals of
order 1; its block is the worst conditioned of all.)  The asserted bounds are 8 x the worst of each column pair:
1.6e-12 on gamma, 1.1e-11 on dx, 4.8e-12 on P+."""
import numpy as np
import pytest

import prior_ref as pr
from msckf_amd import synth
from oracle import msckf_oracle as oracle

BOUND_GAMMA, BOUND_DX, BOUND_P = 8 * 2.0e-13, 8 * 1.3e-12, 8 * 6.0e-13
CASES = [(n, am, False) for n in pr.SHAPES for am in (False, True)] + [("band", False, True), ("band", True, True)]


@pytest.fixture(scope="module")
def shapes():
    return {n: pr.make_shape(n) for n in pr.SHAPES}


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_shapes_are_what_the_gpu_cases_need(shapes):
    for name, prob in shapes.items():
        lens = prob.view_ptr[1:] - prob.view_ptr[:-1]
        has = pr.shape_priors(name, prob).has.astype(bool)
        assert has.any() and lens[has].max() <= 30, name
    lens = lambda n: shapes[n].view_ptr[1:] - shapes[n].view_ptr[:-1]
    has = lambda n: pr.shape_priors(n, shapes[n]).has.astype(bool)
    assert lens("one_view").max() == 1 and has("one_view").all()
    assert lens("band")[has("band")].max() == 10                             # 23 rows, the last of the 24-row instance
    assert set(lens("tiles90")[has("tiles90")]) == {11, 12, 13, 14, 15}      # across the 31- / 33-row boundary
    assert lens("thirty").min() == 30
    assert lens("split_beside").max() > 10 and lens("split_beside")[has("split_beside")].max() <= 10
    assert lens("split_beside_long")[has("split_beside_long")].max() > 10
    assert not pr.SEED_SKIPS                                                 # (a skipped seed is listed there)


@pytest.mark.parametrize("name,at_mean,het", CASES)
def test_the_two_forms_agree(shapes, name, at_mean, het):
    prob = shapes[name]
    pri = pr.shape_priors(name, prob, at_mean)
    vs = pr.het_sigma(prob, pr.shape_seed(name) + 1) if het else None
    a, b = pr.update(prob, pri, vs, "augmented"), pr.update(prob, pri, vs, "inflated")
    assert a["status"] == 0 and b["status"] == 0
    assert pr.clear_of_threshold(a) and pr.clear_of_threshold(b)             # the seed's condition
    assert np.array_equal(a["accepted"], b["accepted"]) and a["n_rejected"] == b["n_rejected"]
    assert np.array_equal(a["crit"], b["crit"])
    e_g = float(np.max(np.abs(a["gamma"] - b["gamma"]) / np.abs(b["gamma"])))
    e_dx, e_P = _rel(a["dx"], b["dx"]), _rel(a["P_new"], b["P_new"])
    print(f"{name} at_mean={at_mean} het={het}: gamma {e_g:.2e}  dx {e_dx:.2e}  P+ {e_P:.2e}")
    assert e_g <= BOUND_GAMMA and e_dx <= BOUND_DX and e_P <= BOUND_P, (e_g, e_dx, e_P)


@pytest.mark.parametrize("name", list(pr.SHAPES))
def test_a_moved_mean_is_rejected_and_a_drawn_one_accepted(shapes, name):
    prob = shapes[name]
    pri = pr.shape_priors(name, prob)
    has = pri.has.astype(bool)
    out = pr.update(prob, pri)
    first = int(np.argmax(has))                                              # the track draw_priors moved
    assert out["accepted"][first] == 0 and out["gamma"][first] > out["crit"][first]
    assert out["accepted"][has].sum() >= 1
    d2 = pr.prior_distance(prob, pri)
    assert np.all(d2[~has] == 0.0) and d2[first] > 100.0 and np.all(d2[has] > 0.0)
    d2m = pr.prior_distance(prob, pr.shape_priors(name, prob, at_mean=True))
    assert np.all(d2m <= 1e-20)                                              # at the mean: 0 to rounding


@pytest.mark.parametrize("name", ["one_chunk", "band"])
def test_all_plain_priors_are_the_oracle(shapes, name):
    prob = shapes[name]
    ref = oracle.update(prob)
    F = prob.F
    none = synth.PointPriors(np.zeros(F, dtype=np.uint8), np.zeros((F, 3)), np.zeros((F, 3, 3)))
    for pri in (None, none):
        for form in ("augmented", "inflated"):
            out = pr.update(prob, pri, form=form)
            assert out["status"] == ref["status"] and np.array_equal(out["accepted"], ref["accepted"])
            assert np.array_equal(out["gamma"], ref["gamma"]) and np.array_equal(out["crit"], ref["crit"])
            if form == "augmented":                                          # the oracle's statements, one by one
                assert np.array_equal(out["dx"], ref["dx"]) and np.array_equal(out["P_new"], ref["P_new"])
            else:                                                            # one dense gain instead of the QR-compressed one
                assert _rel(out["dx"], ref["dx"]) <= BOUND_DX and _rel(out["P_new"], ref["P_new"]) <= BOUND_P


def test_one_view_is_a_no_op_without_priors_and_updates_with(shapes):
    prob = shapes["one_view"]
    assert oracle.update(prob)["status"] == 1                                # 2M - 3 < 0: no rows (MSCKF.py:584-585)
    plain = pr.update(prob, None)
    assert plain["status"] == 1 and not plain["dx"].any() and np.array_equal(plain["P_new"], prob.P)
    out = pr.update(prob, pr.shape_priors("one_view", prob))
    assert out["status"] == 0 and out["accepted"].sum() >= 1 and np.linalg.norm(out["dx"]) > 0
    assert np.all(np.linalg.eigvalsh(prob.P - out["P_new"]) > -1e-12)        # information was added


def test_a_prior_too_loose_to_see_is_rejected(shapes):
    prob = shapes["one_view"]
    pri = pr.shape_priors("one_view", prob)
    pri.cov[3] = 1e40 * np.eye(3)
    rest = np.array([j for j in range(prob.F) if j != 3])
    for form in ("augmented", "inflated"):
        out = pr.update(prob, pri, form=form)
        ref = pr.update(prob.take(rest), pri.take(rest), form=form)
        assert out["accepted"][3] == 0 and out["n_rejected"] == ref["n_rejected"] + 1
        assert np.array_equal(out["dx"], ref["dx"]) and np.array_equal(out["P_new"], ref["P_new"])


def test_pack_helpers():
    from types import SimpleNamespace
    from msckf_amd import pack
    base, point = np.array([0.3, -1.2, 0.5]), np.array([4.0, 2.5, -0.7])
    m, rho = pack.idp_from_point(point, base)
    assert abs(np.linalg.norm(m) - 1.0) < 1e-15 and np.allclose(base + m / rho, point, rtol=0, atol=1e-15)
    sub = pr.at_mean_point(point, base)                       # the device's substitution is the same point
    assert np.array_equal(sub[0], m) and sub[1] == rho
    with pytest.raises(ValueError):
        pack.idp_from_point(base, base)
    feats = {k: SimpleNamespace(keypoints=[0, 1]) for k in ("a", 7, "c")}
    S = np.diag([0.01, 0.04, 0.09])
    pri = pack.point_priors_from_reference(feats, {7: (point, S)}, at_mean=True)
    assert pri.has.tolist() == [0, 1, 0] and np.array_equal(pri.mean[1], point) and np.array_equal(pri.cov[1], S) and pri.at_mean
    with pytest.raises(ValueError):
        pack.point_priors_from_reference(feats, {"zz": (point, S)})


def test_slicing_carries_the_priors(shapes):
    prob = shapes["band"]
    pri = pr.shape_priors("band", prob, at_mean=True)
    full = pr.update(prob, pri)
    carried = type(prob)(**{**prob.__dict__, "point_prior": pri})
    idx = np.array([17, 4, 60, 5, 0, 33])
    for part, sel in ((carried.take(idx), idx), (carried.subset(10, 31), np.arange(10, 31))):
        pp = part.point_prior
        assert pp.F == part.F and pp.at_mean
        assert np.array_equal(pp.has, pri.has[sel]) and np.array_equal(pp.mean, pri.mean[sel]) and np.array_equal(pp.cov, pri.cov[sel])
        out = pr.update(part, pp)
        assert np.array_equal(out["gamma"], full["gamma"][sel]) and np.array_equal(out["accepted"], full["accepted"][sel])
    both = synth.concat_problems(carried.subset(0, 10), prob.subset(10, 20))  # (a side without priors: plain tracks)
    assert np.array_equal(both.point_prior.has, np.concatenate([pri.has[:10], np.zeros(10, dtype=np.uint8)]))
    assert prob.take(idx).point_prior is None
