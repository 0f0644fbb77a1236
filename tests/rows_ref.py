"""Direct measurement rows (msckf_run_rows): the NumPy reference and the one table of cases.  Host only; not a conftest:
imported by name.

The reference project has no such path (its `MSCKF.update` takes camera tracks only), so the yardstick is its own update
algebra, `MSCKF.py:604-614`, stated here for a caller-given H, r and R:

  update(P, H, r, R, crit)   the literal form: inv(S), K = P H^T inv(S), the (I - K H) Joseph product + K R K^T, symmetrised
  update_chol(...)           the engine's form in exact fp64: S = L L^T, W = K S - Y, Pn = P - K Y^T + W K^T
  update_seq(...)            diagonal R only: m sequential one-row Joseph updates
The last two exist to measure the reference spread (tests/test_rows_ref.py): how far exact fp64 algorithms are apart on a case
bounds what a tolerance on that case can mean.

The priors are `filter_prior.filter_prior(N)`: singular, filter-shaped, sigma ratio up to 3e4.  The noise of every case is given
in units of the prior, s = sqrt(diag P), so that no case is a no-information update (an absolute 0.1 m position noise on these
priors missed the spread condition by three decades).  In every case r = chol(S) N(0, I): gamma ~ chi2(m).

  zupt      columns 6..8 (velocity), n_cols = 9, R = diag((f s)^2), f = 0.5
  pos       columns 3..5, n_cols = 6, R = D (A A^T / 3 + f^2 I) D, D = diag(s[3:6]), A standard normal, f = 0.5
  tpos      the same on columns 12..14, n_cols = 15: the columns msckf_run_fix's position fix measures (the error state is
            ordered theta, b_g, v, b_a, p)
  clone     the newest clone's 6 columns, n_cols = d, full R scaled the same way
  imu_m     m standard-normal rows on 15 columns, R_ii = (0.3 |h_i| . s)^2 U(0.5, 2)
  dense_m   m rows on all d columns, entries N(0, 1) / s_j, R_ii = (h_i P h_i^T) U(0.25, 4)
"""
import functools
from collections import namedtuple

import numpy as np

import filter_prior as fp

N_VALUES = (0, 1, 3, 30)                 # d = 15, 21, 33, 195: one ragged tile, two tiles, two tiles + one column, the headline
N_WIDE = 221                             # d = 1341, once: dense_32 and zupt
M_VALUES = (1, 3, 6, 15, 16, 17, 32)     # both sides of the 16-row tile
SPREAD_TOL = 1e-12
MIN_UPDATE = 1e-5

Case = namedtuple("Case", "name kind N m gate")     # gate: None, "above" / "below" (crit = gamma (1 +- 1e-3)) or "table" (chi2_table()[m])

SEED_BASE = {"zupt": 23000, "pos": 23300, "tpos": 23600, "clone": 23900, "imu": 24200, "dense": 24500}
# Seeds follow tests/filter_prior.py's rule: base + N + 1000 k (the generator is seeded [seed, m]) with the first k at which the
# case meets every condition of tests/test_rows_ref.py.  Every case whose k is not 0, with what k = 0 .. missed:
SEED_SKIPS = {}
# Cases whose noise factor f was halved because the case missed the spread condition at f (rather than hunting seeds):
NOISE_FACTOR = {}
GATE_REL = 1e-3


def _cases():
    out = []
    add = lambda kind, N, m, gate=None, tag="": out.append(Case(f"{kind}{'_%d' % m if kind in ('imu', 'dense') else ''}_N{N}{tag}", kind, N, m, gate))
    for N in N_VALUES:
        add("zupt", N, 3)
        add("pos", N, 3)
        add("tpos", N, 3)
        if N >= 1:
            add("clone", N, 6)
        for m in M_VALUES:
            add("imu", N, m)
            add("dense", N, m)
    add("dense", N_WIDE, 32)
    add("zupt", N_WIDE, 3)
    for kind, m in (("imu", 6), ("dense", 17)):          # the gate: both sides of the critical value, and the table's entry
        add(kind, 30, m, "above", "_above")
        add(kind, 30, m, "below", "_below")
    add("zupt", 30, 3, "table", "_table")
    add("imu", 30, 15, "table", "_table")
    return {c.name: c for c in out}


CASES = _cases()


def case_seed(case, k=None):
    return SEED_BASE[case.kind] + case.N + 1000 * (SEED_SKIPS.get(case.name, (0,))[0] if k is None else k)


def _full_noise(rng, s, f):
    A = rng.standard_normal((s.size, s.size))
    return np.diag(s) @ (A @ A.T / 3.0 + f * f * np.eye(s.size)) @ np.diag(s)


def rows_on(P, kind, m, rng, f=0.5):
    """(H, r, R) of a measurement of `kind` with m rows on ANY prior P, sized in units of sqrt(diag P) as the table above says;
    H is m x n_cols.  `measurement` is this on filter_prior(N); tests/call_sequences.py calls it on the P a sequence holds."""
    d = P.shape[0]
    s = np.sqrt(np.diag(P))
    if kind in ("zupt", "pos", "tpos"):
        c0 = {"zupt": 6, "pos": 3, "tpos": 12}[kind]
        H = np.zeros((3, c0 + 3))
        H[:, c0:] = np.eye(3)
        R = np.diag((f * s[c0:c0 + 3]) ** 2) if kind == "zupt" else _full_noise(rng, s[c0:c0 + 3], f)
    elif kind == "clone":
        H = np.zeros((6, d))
        H[:, d - 6:] = np.eye(6)
        R = _full_noise(rng, s[d - 6:], f)
    elif kind == "imu":
        H = rng.standard_normal((m, 15))
        R = np.diag((0.3 * (np.abs(H) @ s[:15])) ** 2 * rng.uniform(0.5, 2.0, m))
    else:
        H = rng.standard_normal((m, d)) / s[None, :]
        R = np.diag(np.einsum("ij,jk,ik->i", H, P, H) * rng.uniform(0.25, 4.0, m))
    R = (R + R.T) / 2                       # bitwise symmetric, as the ABI asks
    Hd = pad(H, d)
    S = Hd @ P @ Hd.T + R
    r = np.linalg.cholesky((S + S.T) / 2) @ rng.standard_normal(H.shape[0])
    return H, r, R


def measurement(case, k=None):
    """(P, H, r, R) of a case; H is m x n_cols."""
    P = np.array(fp.filter_prior(case.N)[0])
    rng = np.random.default_rng([case_seed(case, k), case.m])
    H, r, R = rows_on(P, case.kind, case.m, rng, NOISE_FACTOR.get(case.name, 0.5))
    return P, H, r, R


def pad(H, d):
    H = np.atleast_2d(np.asarray(H, dtype=np.float64))
    out = np.zeros((H.shape[0], d))
    out[:, :H.shape[1]] = H
    return out


def _gated(P, gamma, crit, dx, P_new):
    applied = bool(gamma <= crit)           # (a NaN gamma fails the comparison)
    if not applied:
        dx, P_new = np.zeros(P.shape[0]), np.array(P)
    return dict(status=0 if applied else 1, applied=applied, gamma=float(gamma), dx=dx, P_new=P_new)


def update(P, H, r, R, crit=np.inf):
    """MSCKF.py:604-614 with R in the place of R_n, literally."""
    P = np.asarray(P, dtype=np.float64)
    d = P.shape[0]
    H, r, R = pad(H, d), np.asarray(r, dtype=np.float64).reshape(-1), np.asarray(R, dtype=np.float64)
    S = H @ P @ H.T + R                                      # :604
    Sinv = np.linalg.inv(S)
    K = P @ H.T @ Sinv                                       # :605
    dx = K @ r                                               # :607
    A = np.eye(d) - K @ H                                    # :612
    Pn = A @ P @ A.T + K @ R @ K.T                           # :613
    return _gated(P, r @ Sinv @ r, crit, dx, (Pn + Pn.T) / 2)    # :614


def update_chol(P, H, r, R, crit=np.inf):
    """The engine's form (k_rows.h) in exact fp64."""
    P = np.asarray(P, dtype=np.float64)
    d = P.shape[0]
    H, r, R = pad(H, d), np.asarray(r, dtype=np.float64).reshape(-1), np.asarray(R, dtype=np.float64)
    Y = P @ H.T
    S = H @ Y + R
    L = np.linalg.cholesky(S)
    w = np.linalg.solve(L, r)
    K = np.linalg.solve(L.T, np.linalg.solve(L, Y.T)).T
    W = K @ S - Y
    Pn = P - K @ Y.T + W @ K.T
    return _gated(P, w @ w, crit, K @ r, (Pn + Pn.T) / 2)


def update_seq(P, H, r, R, crit=np.inf):
    """Diagonal R: m one-row Joseph updates in turn.  (I - k h) P (I - k h)^T + k R_ii k^T is expanded around the row so that
    a step costs d^2, not d^3; gamma is that of the joint form, the sum of the rows' innovations squared over their variances."""
    P0 = np.asarray(P, dtype=np.float64)
    d = P0.shape[0]
    H, r, R = pad(H, d), np.asarray(r, dtype=np.float64).reshape(-1), np.asarray(R, dtype=np.float64)
    assert np.count_nonzero(R - np.diag(np.diag(R))) == 0
    Pk, x, gamma = np.array(P0), np.zeros(d), 0.0
    for i in range(H.shape[0]):
        h = H[i]
        y = Pk @ h
        yt = h @ Pk
        q = h @ y
        s = q + R[i, i]
        k = y / s
        e = r[i] - h @ x
        gamma += e * e / s
        x = x + k * e
        Pk = Pk - np.outer(k, yt) - np.outer(y, k) + np.outer(k, k) * (q + R[i, i])
        Pk = (Pk + Pk.T) / 2
    return _gated(P0, gamma, crit, x, Pk)


def critical(case, gamma):
    """The critical value a gated case runs with (None: not gated), from the reference gamma."""
    if case.gate is None:
        return None
    if case.gate == "table":
        from msckf_amd.api import chi2_table
        return float(chi2_table()[case.m])
    return float(gamma * (1 + GATE_REL)) if case.gate == "above" else float(gamma * (1 - GATE_REL))


@functools.lru_cache(maxsize=None)
def problem(name, k=None):
    """((P, H, r, R), crit, reference result) of a case, computed once and shared: leave all of it unchanged."""
    case = CASES[name]
    P, H, r, R = measurement(case, k)
    free = update(P, H, r, R)
    crit = critical(case, free["gamma"])
    ref = free if crit is None else update(P, H, r, R, crit)
    for a in (P, H, r, R, ref["dx"], ref["P_new"]):
        a.setflags(write=False)
    return (P, H, r, R), crit, ref


def spread(name, k=None):
    """The largest of filter_prior.metrics over the other exact forms against `update`, without the gate."""
    (P, H, r, R), _, _ = problem(name, k)
    ref = update(P, H, r, R)
    forms = [update_chol]
    if np.count_nonzero(R - np.diag(np.diag(R))) == 0:
        forms.append(update_seq)
    worst = np.zeros(5)
    for form in forms:
        got = form(P, H, r, R)
        worst = np.maximum(worst, fp.metrics(got["dx"], got["P_new"], ref, P))
    return tuple(float(x) for x in worst)


def removed(name, k=None):
    """|P - P+| / |P| of the ungated update."""
    (P, H, r, R), _, _ = problem(name, k)
    ref = update(P, H, r, R)
    return float(np.linalg.norm(P - ref["P_new"]) / np.linalg.norm(P))
