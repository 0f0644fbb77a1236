"""The update with priors on the tracks' points, restated in NumPy from the oracle's own pieces.

A track whose point is known as p ~ N(pbar, Sigma_p) (csrc/point_prior.h), in two forms that must agree:

  "augmented"  three rows [sigma W | 0 | sigma W (pbar - p_lin)], W = L^-1 of Sigma_p = L L^T and p_lin = base + m / rho,
               behind the track's [H_f | H_x | r] of `oracle.feature_blocks`, then the oracle's own
               `project_on_nullspace` (2M + 3 rows, 2M left) and `gate` with the global sigma, then stacking, QR
               compression, gain and Joseph form as `oracle.update` writes them (`MSCKF.py:594-614`): what the device does;
  "inflated"   the EKF update with residual r - H_f (pbar - p_lin), Jacobian H_x and noise sigma^2 I + H_f Sigma_p H_f^T
               on the track's 2M rows, gated at 2M degrees of freedom, in one dense gain over the stacked rows with
               block-diagonal noise: the statement of what a prior on the point means.

Per-view weights w_v = sigma / sigma_v scale the views' rows in front of either form (tests/weighted_ref.py); prior rows
are not weighted.  `at_mean`: a prior track is linearised at m' = (pbar - base) rho', rho' = 1 / |pbar - base| in place of
its own m, rho (where |pbar - base| is finite and not 0)."""
import numpy as np
from scipy.linalg import null_space
from scipy.stats import chi2

from oracle import msckf_oracle as oracle
from weighted_ref import clear_of_threshold, het_sigma, view_weights  # noqa: F401  (re-exported to the tests)


def whitening(cov):
    """W = L^-1, lower triangular, of cov = L L^T."""
    L = np.linalg.cholesky(np.asarray(cov, dtype=np.float64))
    return np.linalg.solve(L, np.eye(3))


def at_mean_point(mean, base):
    """(m', rho') of the linearise-at-the-mean substitution, or None where the track keeps its own point."""
    d = np.asarray(mean, dtype=np.float64) - np.asarray(base, dtype=np.float64)
    n = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    if not np.isfinite(n) or n == 0.0 or not np.isfinite(1.0 / n):
        return None
    return d * (1.0 / n), 1.0 / n


def linearised(prob, priors):
    """`prob` with the m, rho every K1 term of the run is formed from: the at-mean substitution on the prior tracks."""
    if priors is None or not priors.at_mean:
        return prob
    m, rho = prob.idp_m.copy(), prob.idp_rho.copy()
    for j in np.nonzero(priors.has)[0]:
        sub = at_mean_point(priors.mean[j], prob.idp_base[j])
        if sub is not None:
            m[j], rho[j] = sub
    return type(prob)(**{**prob.__dict__, "idp_m": m, "idp_rho": rho})


def p_lin(prob, j):
    return prob.idp_base[j] + prob.idp_m[j] / prob.idp_rho[j]


def prior_rows(prob, priors, j):
    """(h (3, 3), res (3,)) of track j's prior block at `prob`'s linearisation point: sigma W, sigma W (pbar - p_lin)."""
    sW = float(prob.sigma) * whitening(priors.cov[j])
    return sW, sW @ (priors.mean[j] - p_lin(prob, j))


def prior_distance(prob, priors):
    """(pbar - p_lin)^T Sigma_p^-1 (pbar - p_lin) per track at the run's linearisation point, 0 for a plain track."""
    lin = linearised(prob, priors)
    out = np.zeros(prob.F)
    for j in np.nonzero(priors.has)[0]:
        y = whitening(priors.cov[j]) @ (priors.mean[j] - p_lin(lin, j))
        out[j] = float(y @ y)
    return out


def _weighted_blocks(prob, w, j):
    a = int(prob.view_ptr[j])
    r, H_x, H_f = oracle.feature_blocks(prob, j)
    w2 = np.repeat(w[a:a + r.shape[0] // 2], 2)          # both rows of a view
    return w2 * r, w2[:, None] * H_x, w2[:, None] * H_f


def _finish(P, sigma, accepted, gammas, crits, H_list, r_list, R_list):
    """Stacking, gain and Joseph form.  R_list None: every row at sigma^2 (the oracle's path, QR-compressed where m > d);
    else the rows' noise blocks, one dense gain."""
    d, F = P.shape[0], accepted.shape[0]
    out = dict(status=1, dx=np.zeros(d), P_new=P.copy(), accepted=accepted, gamma=gammas, crit=crits,
               n_rejected=int(np.sum(accepted == 0)))
    if not H_list:                                           # MSCKF.py:584-585
        return out
    H_X = np.vstack(H_list)
    r_o = np.concatenate(r_list)
    m = H_X.shape[0]
    if m == 0:                                               # :591-592
        return out
    if R_list is None:
        if m > d:                                            # :594-598
            Q, R = np.linalg.qr(H_X, mode="reduced")
            T_H, r_n, R_n = R, Q.T @ r_o, sigma ** 2 * np.eye(d)
        else:                                                # :599-602
            T_H, r_n, R_n = H_X, r_o, sigma ** 2 * np.eye(m)
    else:
        T_H, r_n = H_X, r_o
        R_n = np.zeros((m, m))
        i = 0
        for Rb in R_list:
            R_n[i:i + Rb.shape[0], i:i + Rb.shape[0]] = Rb
            i += Rb.shape[0]
    S = T_H @ P @ T_H.T + R_n                                # :605
    Kg = np.linalg.solve(S, T_H @ P).T if R_list is not None else P @ T_H.T @ np.linalg.inv(S)   # :606
    dx = Kg @ r_n                                            # :607
    I = np.eye(d)
    Pn = (I - Kg @ T_H) @ P @ (I - Kg @ T_H).T + Kg @ R_n @ Kg.T  # :613
    Pn = (Pn + Pn.T) / 2                                     # :614
    out.update(status=0, dx=dx, P_new=Pn)
    return out


def update(prob, priors, view_sigma=None, form="augmented"):
    """dict(status, dx, P_new, accepted, gamma, crit, n_rejected) like `oracle.update`.  `priors`: synth.PointPriors or
    None (every track plain).  A prior track whose augmented block has rank < 3 (a prior so loose that sigma W vanishes
    beside H_f) would leave more than 2M rows: it is rejected, in both forms."""
    assert form in ("augmented", "inflated")
    P, F, sigma = prob.P, prob.F, float(prob.sigma)
    w = view_weights(prob, view_sigma)
    lin = linearised(prob, priors)
    accepted = np.zeros(F, dtype=np.uint8)
    gammas, crits = np.zeros(F), np.zeros(F)
    H_list, r_list, R_list = [], [], []
    for j in range(F):                                       # MSCKF.py:573
        r, H_x, H_f = _weighted_blocks(lin, w, j)
        R_j = None
        if priors is not None and priors.has[j]:
            sW, pres = prior_rows(lin, priors, j)
            H_aug = np.vstack([H_f, sW])
            if null_space(H_aug.T).shape[1] != r.shape[0]:   # rank < 3: not stacked, counted as rejected
                crits[j] = float(chi2.ppf(0.95, r.shape[0]))
                continue
            if form == "augmented":
                r_o, H_o = oracle.project_on_nullspace(H_aug, np.concatenate([r, pres]),
                                                       np.vstack([H_x, np.zeros((3, H_x.shape[1]))]))
                ok, gammas[j], crits[j] = oracle.gate(r_o, H_o, P, sigma)
            else:
                r_o = r - H_f @ (priors.mean[j] - p_lin(lin, j))
                H_o = H_x
                R_j = sigma ** 2 * np.eye(r.shape[0]) + H_f @ priors.cov[j] @ H_f.T
                gammas[j] = float(r_o @ np.linalg.solve(H_o @ P @ H_o.T + R_j, r_o))
                crits[j] = float(chi2.ppf(0.95, r.shape[0]))
                ok = gammas[j] <= crits[j]
        else:
            r_o, H_o = oracle.project_on_nullspace(H_f, r, H_x)
            ok, gammas[j], crits[j] = oracle.gate(r_o, H_o, P, sigma)
            R_j = sigma ** 2 * np.eye(r_o.shape[0])
        if not ok:
            continue                                         # :577-579
        accepted[j] = 1
        H_list.append(H_o)
        r_list.append(r_o)
        R_list.append(R_j)
    return _finish(P, sigma, accepted, gammas, crits, H_list, r_list, None if form == "augmented" else R_list)


# ---- the GPU cases (tests/test_gpu_point_priors.py) -------------------------------------------------------------------------
# name -> (N, F, M, make_problem's switches, engine plan, which tracks carry priors); the smallest shapes at which the prior
# form of K1-K4 takes another path
SHAPES = {
    "one_view": (4, 8, 1, {"min_track": 1}, "auto", "all"),                        # rows from tracks that gave none; M = 1 blocks
    "one_chunk": (8, 24, 6, {}, "auto", "half"),                                   # 15 rows in the 24-row instance
    "band": (30, 120, 10, {"variable_tracks": True}, "auto", "half"),              # up to 23 rows, the last of the 24-row instance
    "tiles90": (30, 100, 15, {"variable_tracks": True}, "band", "from11"),         # 25..33 rows: the 32- / 64-row boundary
    "thirty": (31, 8, 30, {}, "auto", "half"),                                     # 63 rows on 64 lanes
    "split_beside": (20, 40, 20, {"variable_tracks": True, "min_track": 2}, "auto", "short"),   # long plain tracks split beside
    "split_beside_long": (20, 40, 20, {"variable_tracks": True, "min_track": 2}, "auto", "short+1"),   # ... and one long prior track
}
# Seeds: the first seed from SEED_BASE + (index of the shape) for which, with the priors of `draw_priors` in both forms, as they
# are and linearised at the mean (and, on "band", under the heterogeneous view_sigma draw), the restatement updates (status 0)
# and no track's |gamma - crit| < 1e-6 crit.  Seeds that were skipped: SEED_SKIPS (shape -> seeds).
SEED_BASE = 9300
SEED_SKIPS = {}
STD_RANGE = (0.01, 0.30)                                                           # principal standard deviations, metres
FAR = 10.0                                                                         # metres a "moved" mean lies off its draw


def shape_seed(name):
    return SEED_BASE + list(SHAPES).index(name) + 100 * len(SEED_SKIPS.get(name, ()))


def make_shape(name):
    from msckf_amd import synth
    N, F, M, kw, _, _ = SHAPES[name]
    return synth.make_problem(N, F, M, seed=shape_seed(name), **kw)


def prior_tracks(prob, which):
    lens = np.asarray(prob.view_ptr[1:] - prob.view_ptr[:-1])
    F = prob.F
    if which == "all":
        return np.ones(F, dtype=bool)
    if which == "half":
        return np.arange(F) % 2 == 0
    if which == "from11":                                    # prior tracks of 11 to 15 views; shorter ones stay plain
        return lens >= 11
    has = (lens <= 10) & (np.arange(F) % 2 == 0)             # "short": the long tracks stay plain (and are split)
    if which == "short+1":
        has[int(np.argmax(lens > 10))] = True
    return has


def draw_priors(prob, seed, which="half", at_mean=False):
    """Sigma_p = L L^T with L = Q diag(s), Q a random rotation and s log-uniform in STD_RANGE; mean = p_lin + L z.  The first
    prior track's mean is then moved FAR metres across its bearing (a landmark matched to the wrong map point: the gate must
    refuse it), the others stay where they were drawn."""
    from msckf_amd import synth
    rng = np.random.default_rng(seed)
    F = prob.F
    has = prior_tracks(prob, which)
    mean, cov = np.zeros((F, 3)), np.zeros((F, 3, 3))
    moved = False
    for j in range(F):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        s = np.exp(rng.uniform(np.log(STD_RANGE[0]), np.log(STD_RANGE[1]), 3))
        z = rng.standard_normal(3)
        if not has[j]:
            continue
        L = Q * s
        C = L @ L.T
        cov[j] = (C + C.T) / 2
        mean[j] = p_lin(prob, j) + L @ z
        if not moved:
            across = np.cross(prob.idp_m[j], [0.0, 0.0, 1.0])
            mean[j] += FAR * across / np.linalg.norm(across)
            moved = True
    return synth.PointPriors(has.astype(np.uint8), mean, cov, at_mean)


def shape_priors(name, prob=None, at_mean=False):
    prob = make_shape(name) if prob is None else prob
    return draw_priors(prob, shape_seed(name) + 7, SHAPES[name][5], at_mean)
