"""tests/weighted_ref.py -- the NumPy restatement of the update with per-view noise -- against the oracle where the two must
agree, the declarations of the two symbols, and the seed rule of the GPU cases (tests/test_gpu_view_sigma.py).  CPU only."""
import os
import re

import numpy as np
import pytest

import weighted_ref as wr
from conftest import ROOT, rel_err
from msckf_amd import synth
from oracle import msckf_oracle as oracle

# (the basis of a track's null space differs between diag(w) H_f and H_f by rounding only when w is uniform: 1e-12 holds the
#  two updates together, as it holds the oracle's dense and analytic noise forms together)
TOL = 1e-12


def _small():
    return synth.make_problem(8, 24, 6, seed=3, outlier_fraction=0.1, outlier_px=500.0)


@pytest.mark.parametrize("c", [0.5, 2.0, 3.0])
def test_uniform_weights_equal_the_oracle_at_the_scaled_sigma(c):
    """sigma_v = sigma / c for every view == the unweighted update with the global sigma / c."""
    prob = _small()
    vs = np.full(int(prob.view_ptr[-1]), prob.sigma / c)
    out = wr.update(prob, vs)
    scaled = synth.UpdateProblem(**{**prob.__dict__, "sigma": prob.sigma / c})
    ref = oracle.update(scaled, dense_noise=False)
    assert out["status"] == ref["status"] == 0
    assert np.array_equal(out["accepted"], ref["accepted"]) and 0 < int(ref["accepted"].sum()) < prob.F
    assert np.allclose(out["gamma"], ref["gamma"], rtol=1e-9, atol=0.0)
    assert rel_err(out["dx"], ref["dx"]) < TOL and rel_err(out["P_new"], ref["P_new"]) < TOL


def test_all_ones_equal_the_oracle():
    prob = _small()
    out = wr.update(prob, np.full(int(prob.view_ptr[-1]), prob.sigma))
    assert np.all(wr.view_weights(prob, np.full(int(prob.view_ptr[-1]), prob.sigma)) == 1.0)
    ref = oracle.update(prob, dense_noise=False)
    assert out["status"] == ref["status"] == 0 and np.array_equal(out["accepted"], ref["accepted"])
    assert np.array_equal(out["gamma"], ref["gamma"])
    assert rel_err(out["dx"], ref["dx"]) < TOL and rel_err(out["P_new"], ref["P_new"]) < TOL
    none = wr.update(prob)
    assert np.array_equal(none["dx"], out["dx"]) and np.array_equal(none["P_new"], out["P_new"])


def test_whitened_form_is_the_R_o_form():
    """Heterogeneous weights against the update written with R_o = blockdiag(sigma_v^2 I_2) itself: per track the null space of
    the UNWEIGHTED H_f, the projected noise A^T R_j A in the gate and in the stacked system (no compression: m <= d)."""
    prob = synth.make_problem(8, 12, 4, seed=5)
    vs = wr.het_sigma(prob, 1)
    out = wr.update(prob, vs)
    P, d = prob.P, prob.P.shape[0]
    H_list, r_list, R_list = [], [], []
    gam = np.zeros(prob.F)
    for j in range(prob.F):
        a, b = int(prob.view_ptr[j]), int(prob.view_ptr[j + 1])
        r, H_x, H_f = oracle.feature_blocks(prob, j)
        A = oracle.null_space(H_f.T)
        Rj = A.T @ np.diag(np.repeat(vs[a:b], 2) ** 2) @ A
        r_o, H_o = A.T @ r, A.T @ H_x
        gam[j] = float(r_o @ np.linalg.inv(H_o @ P @ H_o.T + Rj) @ r_o)
        if out["accepted"][j]:
            H_list.append(H_o); r_list.append(r_o); R_list.append(Rj)
    assert np.allclose(gam, out["gamma"], rtol=1e-9, atol=0.0)
    H, r = np.vstack(H_list), np.concatenate(r_list)
    m = H.shape[0]
    assert 0 < m <= d
    Rn = np.zeros((m, m))
    o = 0
    for Rj in R_list:
        Rn[o:o + Rj.shape[0], o:o + Rj.shape[0]] = Rj
        o += Rj.shape[0]
    Kg = P @ H.T @ np.linalg.inv(H @ P @ H.T + Rn)
    I = np.eye(d)
    Pn = (I - Kg @ H) @ P @ (I - Kg @ H).T + Kg @ Rn @ Kg.T
    assert out["status"] == 0
    assert rel_err(out["dx"], Kg @ r) < 1e-9 and rel_err(out["P_new"], (Pn + Pn.T) / 2) < 1e-9


def test_problem_carries_view_sigma_through_take_and_subset():
    prob = _small()
    assert prob.view_sigma is None and prob.subset(2, 5).view_sigma is None and prob.take([1, 3]).view_sigma is None
    prob.view_sigma = wr.het_sigma(prob, 2)
    vp = prob.view_ptr
    sub = prob.subset(2, 5)
    assert np.array_equal(sub.view_sigma, prob.view_sigma[vp[2]:vp[5]]) and sub.view_sigma.size == sub.view_ptr[-1]
    tk = prob.take([4, 1])
    assert np.array_equal(tk.view_sigma, np.concatenate([prob.view_sigma[vp[4]:vp[5]], prob.view_sigma[vp[1]:vp[2]]]))


def test_reference_shaped_mapping_is_packed_in_keypoint_order():
    from types import SimpleNamespace as NS
    from msckf_amd.pack import view_sigma_from_reference
    feats = {7: NS(keypoints=[0, 1, 2]), 3: NS(keypoints=[0, 1]), 9: NS(keypoints=[0])}
    vs = view_sigma_from_reference(feats, {3: [0.5, 0.25], 7: [1.0, 2.0, 3.0]}, 0.2)
    assert np.array_equal(vs, [1.0, 2.0, 3.0, 0.5, 0.25, 0.2])
    with pytest.raises(ValueError):
        view_sigma_from_reference(feats, {7: [1.0]}, 0.2)


def test_header_and_ffi_declare_the_two_symbols():
    from msckf_amd import _ffi
    with open(os.path.join(ROOT, "include", "msckf_mi355x.h")) as f:
        hdr = f.read()
    assert re.search(r"#define MSCKF_ABI_VERSION 2\b", hdr)
    assert re.search(r"\bint msckf_set_view_sigma\(msckf_ctx\* ctx, const double\* sigma_view\);", hdr)
    m = re.search(r"\bint msckf_update_sigma\(([^;]*)\);", hdr)
    u = re.search(r"\bint msckf_update\(([^;]*)\);", hdr)
    args = lambda s: [a.strip() for a in s.replace("\n", " ").split(",")]
    au, am = args(u.group(1)), args(m.group(1))
    k = au.index("const double* idp_rho")
    assert am == au[:k + 1] + ["const double* sigma_view"] + au[k + 1:]          # msckf_update's signature, the array behind idp_rho
    for name in ("msckf_update_sigma", "msckf_set_view_sigma"):
        assert name in _ffi.SYMBOLS
    with open(os.path.join(ROOT, "monocular-visual-inertial-msckf_amd", "_ffi.py")) as f:
        src = f.read()
    assert "lib.msckf_update_sigma.argtypes" in src and "lib.msckf_set_view_sigma.argtypes" in src


@pytest.mark.parametrize("name", list(wr.SHAPES))
def test_gpu_cases_follow_the_seed_rule(name):
    """Every weighting the GPU tests run on a shape: the restatement updates and no gate decision lies within 1e-6 of its
    threshold -- for the shape's seed, and for none of the seeds listed as skipped."""
    def ok(seed):
        N, F, M, kw, _ = wr.SHAPES[name]
        prob = synth.make_problem(N, F, M, seed=seed, **kw)
        n = int(prob.view_ptr[-1])
        for vs in (None, np.full(n, prob.sigma / 2), wr.het_sigma(prob, seed)):
            out = wr.update(prob, vs)
            if out["status"] != 0 or not wr.clear_of_threshold(out):
                return False
        return True
    assert ok(wr.shape_seed(name))
    for s in wr.SEED_SKIPS.get(name, ()):
        assert not ok(s)
