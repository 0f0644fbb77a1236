"""The robust-weight restatement (tests/robust_ref.py) on the CPU: that every GPU case of tests/test_gpu_view_robust.py is a
case -- the update runs with and without the option, no gate decision sits within rounding of its threshold, the option
rescues a track, it reaches the shape's longest tracks, no Huber decision sits within rounding of k -- and two properties
of the definition: a k beyond every residual is the plain update, and a common scale of the sigmas changes nothing."""
import numpy as np
import pytest

import robust_ref as rr
import weighted_ref as wr
from msckf_amd import synth
from oracle import msckf_oracle as oracle

CASES = [(n, v) for n in rr.SHAPES for v in rr.VARIANTS]


@pytest.mark.parametrize("name,which", CASES)
def test_case_is_admitted(name, which):
    prob = rr.make_shape(name)
    base = rr.plain_ref(name, which == "huber_het")
    out, wt = rr.robust_ref(name, which)
    assert base["status"] == 0 and out["status"] == 0
    assert wr.clear_of_threshold(base) and wr.clear_of_threshold(out)
    resc = rr.rescued(name, which)
    print(name, which, "accepted", int(base["accepted"].sum()), "->", int(out["accepted"].sum()), "rescued", resc.size,
          "n_down", wt["n_down"], "of", wt["s"].size)
    assert resc.size >= 1
    lens = np.diff(prob.view_ptr)
    lo, hi = rr.LONGEST[name]
    assert lens.max() <= hi
    down_per_track = np.add.reduceat((wt["phi"] < 1.0).astype(np.int64), prob.view_ptr[:-1])
    assert np.any((lens >= lo) & (down_per_track > 0))
    if which.startswith("huber"):
        k = rr.variant(name, which)[1]
        assert float(np.min(np.abs(wt["s"] - k))) / k > 1e-6
    # the weights are what the definition says of them
    assert np.all(wt["w"] <= wt["b"]) and np.all(wt["phi"] >= rr.W_MIN) and np.all(wt["s"] >= 0)


@pytest.mark.parametrize("name", ["one_chunk", "split"])
def test_a_huber_k_beyond_every_residual_is_the_plain_update(name):
    prob = rr.make_shape(name)
    s = rr.weights(prob, "huber", rr.HUBER_K, rr.W_MIN)["s"]
    k = 2.0 * float(s.max())
    out, wt = rr.update(prob, "huber", k, rr.W_MIN)
    assert np.array_equal(wt["w"], np.ones(s.size)) and wt["n_down"] == 0
    ref = oracle.update(prob, dense_noise=False)
    assert np.array_equal(out["accepted"], ref["accepted"]) and np.array_equal(out["gamma"], ref["gamma"])
    assert np.array_equal(out["dx"], ref["dx"]) and np.array_equal(out["P_new"], ref["P_new"])


@pytest.mark.parametrize("loss", list(rr.LOSSES))
def test_s_and_phi_depend_on_the_views_own_sigma_alone(loss):
    """s_v = b_v |e_v| / sigma = |e_v| / sigma_v: how a view's noise is split into the global sigma and its base weight does not
    matter.  With the sigma_v held and the global sigma times c, b_v scales by c and s_v, phi_v stay; w_v = b_v phi_v scales by c.
    With sigma_v AND sigma times c (b_v unchanged) the same residual is 1 / c as many sigmas, so s_v scales by 1 / c and phi_v is
    that of the loss at k c.  (c a power of two: the scalings are exact up to the last division.)"""
    name = "band"
    prob = rr.make_shape(name)
    vs = rr.het_sigma(name)
    k = rr.LOSSES[loss]
    w0 = rr.weights(prob, loss, k, rr.W_MIN, vs)
    for c in (0.5, 4.0):
        scaled = synth.UpdateProblem(**{**prob.__dict__, "sigma": prob.sigma * c})
        w1 = rr.weights(scaled, loss, k, rr.W_MIN, vs)
        assert np.array_equal(w1["b"], c * w0["b"])
        assert np.allclose(w1["s"], w0["s"], rtol=4e-16, atol=0.0) and np.allclose(w1["phi"], w0["phi"], rtol=4e-16, atol=0.0)
        assert np.allclose(w1["w"], c * w0["w"], rtol=4e-16, atol=0.0)
        w2 = rr.weights(scaled, loss, k, rr.W_MIN, vs * c)
        assert np.array_equal(w2["b"], w0["b"])
        assert np.allclose(w2["s"] * c, w0["s"], rtol=4e-16, atol=0.0)
        w3 = rr.weights(scaled, loss, k / c, rr.W_MIN, vs * c)
        assert np.allclose(w3["phi"], w0["phi"], rtol=4e-16, atol=0.0)
