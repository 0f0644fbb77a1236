"""Robust per-view weights in front of K1 (`msckf_set_robust`), restated in NumPy from the oracle's own pieces.

Not in the reference: its only defence against a bad observation is the gate (`MSCKF.py:562-579`).  One reweighting at
the linearisation point: with e_v the view's two residual components (`oracle.feature_blocks`: z - z_hat in normalised
image coordinates, `MSCKF.py:516-524`), b_v = sigma / sigma_v the base weight (1 without per-view noise) and
s_v = b_v |e_v| / sigma the whitened residual norm,

    omega(s) = min(1, k / s)  (Huber)   |   1 / (1 + (s / k)^2)  (Cauchy)
    phi_v = max(sqrt(omega(s_v)), w_min)        (1 where s_v is not finite)
    w_v = b_v phi_v

and the update is `weighted_ref.update` with sigma_v' = sigma / w_v: the rows of view v times w_v in front of the
null-space projection, everything behind as the oracle writes it."""
import functools

import numpy as np

import weighted_ref as wr
from oracle import msckf_oracle as oracle

HUBER_K, CAUCHY_K, W_MIN = 1.345, 2.385, 0.05
LOSSES = {"huber": HUBER_K, "cauchy": CAUCHY_K}

# the six shapes of weighted_ref.SHAPES and a wide one (tracks of 28 - 48 views: k_feature_wide among the narrow kernels)
SHAPES = dict(wr.SHAPES)
SHAPES["wide"] = (48, 12, 48, {"variable_tracks": True, "min_track": 28}, "auto")
OUTLIERS = dict(outlier_fraction=0.3, outlier_px=400.0)
# the longest class of each shape: (fewest, most) views of a track that the shape's form is about
LONGEST = {"one_chunk": (6, 6), "band": (8, 10), "tiles90": (11, 15), "ring": (10, 10), "split": (16, 20), "unsplit31": (31, 31),
           "wide": (32, 48)}
# Seeds: the first seed from SEED_BASE, in steps of 1, for which every variant the tests use (Huber, Huber on the heterogeneous
# base, Cauchy) meets the admission conditions of tests/test_robust_ref.py.  Skipped seeds: SEED_SKIPS (shape -> number).
SEED_BASE = 9300
SEED_SKIPS = {}
VARIANTS = ("huber", "huber_het", "cauchy")


def shape_seed(name):
    return SEED_BASE + SEED_SKIPS.get(name, 0)


@functools.lru_cache(maxsize=None)
def make_shape(name):
    from msckf_amd import synth
    N, F, M, kw, _ = SHAPES[name]
    return synth.make_problem(N, F, M, seed=shape_seed(name), **kw, **OUTLIERS)


def het_sigma(name):
    return wr.het_sigma(make_shape(name), shape_seed(name))


def omega(loss, k, s):
    s = np.asarray(s, dtype=np.float64)
    if loss == "huber":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(s <= k, 1.0, k / s)
    if loss == "cauchy":
        with np.errstate(over="ignore", invalid="ignore"):
            return 1.0 / (1.0 + (s / k) ** 2)
    raise ValueError(loss)


def phi(loss, k, w_min, s):
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        p = np.maximum(np.sqrt(omega(loss, k, s)), w_min)
    return np.where(np.isfinite(s), p, 1.0)


def residual_norms(prob):
    """|e_v|_2 per view, input order."""
    n = int(prob.view_ptr[-1])
    out = np.zeros(n)
    for j in range(prob.F):
        a = int(prob.view_ptr[j])
        r, _, _ = oracle.feature_blocks(prob, j)
        e = r.reshape(-1, 2)
        out[a:a + e.shape[0]] = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
    return out


def weights(prob, loss, k, w_min, view_sigma=None):
    """dict(w, s, phi, b, n_down) by the definition above; `view_sigma` None: `prob.view_sigma`, else every view at sigma."""
    b = wr.view_weights(prob, view_sigma)
    s = b * residual_norms(prob) / float(prob.sigma)
    p = phi(loss, k, w_min, s)
    return dict(w=b * p, s=s, phi=p, b=b, n_down=int(np.count_nonzero(p < 1.0)))


def update(prob, loss, k, w_min, view_sigma=None):
    """(`weighted_ref.update`'s dict at sigma_v' = sigma / w_v, the weights' dict)."""
    wt = weights(prob, loss, k, w_min, view_sigma)
    return wr.update(prob, view_sigma=float(prob.sigma) / wt["w"]), wt


def variant(name, which):
    """(loss, k, view_sigma or None) of a test variant of shape `name`."""
    if which == "huber":
        return "huber", HUBER_K, None
    if which == "huber_het":
        return "huber", HUBER_K, het_sigma(name)
    if which == "cauchy":
        return "cauchy", CAUCHY_K, None
    raise ValueError(which)


@functools.lru_cache(maxsize=None)
def plain_ref(name, het=False):
    """The update without the option (on the heterogeneous base where `het`)."""
    return wr.update(make_shape(name), het_sigma(name) if het else None)


@functools.lru_cache(maxsize=None)
def robust_ref(name, which):
    loss, k, vs = variant(name, which)
    return update(make_shape(name), loss, k, W_MIN, vs)


def rescued(name, which):
    """Tracks the gate rejects without the option and accepts with it."""
    out, _ = robust_ref(name, which)
    base = plain_ref(name, which == "huber_het")
    return np.nonzero((base["accepted"] == 0) & (out["accepted"] == 1))[0]


def close(x, ref):
    """The bound on w and s against this helper: |diff| <= 1e-12 (1 + |ref|).  e is a difference of O(1) quantities (|z| <= 2.2 with
    the synthetic K): ~1e-15 absolute; b <= 2 and sigma = 0.2 make that ~1e-14 on s, phi is no steeper than s; a hundred times that."""
    x, ref = np.asarray(x), np.asarray(ref)
    return bool(np.all(np.abs(x - ref) <= 1e-12 * (1.0 + np.abs(ref))))


def worst(x, ref):
    x, ref = np.asarray(x), np.asarray(ref)
    return float(np.max(np.abs(x - ref) / (1.0 + np.abs(ref)))) if x.size else 0.0
