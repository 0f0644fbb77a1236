"""The update with per-view measurement noise, restated in NumPy from the oracle's own pieces.

`MSCKF.update` with R_o = blockdiag(sigma_v^2 I_2) in place of sigma^2 I (reference `MSCKF.py:589`, and `:562` in
the gate), computed in whitened form: with w_v = sigma / sigma_v the two rows of view v of r, H_x and H_f
(`oracle.feature_blocks`) are multiplied by w_v BEFORE the null-space projection (`:550`), and from there on the
oracle's code runs with the global sigma -- the left null space is that of diag(w) H_f, so the projected noise is
sigma^2 I again.  Stacking, QR compression, gain and the Joseph form are `MSCKF.py:594-614` exactly as
`oracle.update` writes them (dense_noise=False)."""
import numpy as np

from oracle import msckf_oracle as oracle


def view_weights(prob, view_sigma=None):
    """w_v = sigma / sigma_v, the fp64 quotient (exactly 1 where sigma_v == sigma); all ones without weights."""
    vs = prob.view_sigma if view_sigma is None else view_sigma
    n = int(prob.view_ptr[-1])
    if vs is None:
        return np.ones(n)
    vs = np.asarray(vs, dtype=np.float64).reshape(-1)
    assert vs.size == n and np.all(np.isfinite(vs)) and np.all(vs > 0)
    return float(prob.sigma) / vs


def update(prob, view_sigma=None):
    """dict(status, dx, P_new, accepted, gamma, crit, n_rejected) like `oracle.update`."""
    P = prob.P
    d = P.shape[0]
    F = prob.F
    sigma = prob.sigma
    w = view_weights(prob, view_sigma)
    accepted = np.zeros(F, dtype=np.uint8)
    gammas = np.zeros(F)
    crits = np.zeros(F)
    H_list, r_list = [], []
    for j in range(F):                                       # MSCKF.py:573
        a = int(prob.view_ptr[j])
        r, H_x, H_f = oracle.feature_blocks(prob, j)
        w2 = np.repeat(w[a:a + r.shape[0] // 2], 2)          # both rows of a view
        r, H_x, H_f = w2 * r, w2[:, None] * H_x, w2[:, None] * H_f
        r_o, H_o = oracle.project_on_nullspace(H_f, r, H_x)
        ok, gammas[j], crits[j] = oracle.gate(r_o, H_o, P, sigma)
        if not ok:
            continue                                         # :577-579
        accepted[j] = 1
        H_list.append(H_o)
        r_list.append(r_o)
    out = dict(status=1, dx=np.zeros(d), P_new=P.copy(), accepted=accepted, gamma=gammas, crit=crits,
               n_rejected=int(F - accepted.sum()))
    if not H_list:                                           # :584-585
        return out
    H_X = np.vstack(H_list)
    r_o = np.concatenate(r_list)
    m = H_X.shape[0]
    if m == 0:                                               # :591-592
        return out
    if m > d:                                                # :594-598
        Q, R = np.linalg.qr(H_X, mode="reduced")
        T_H = R
        r_n = Q.T @ r_o
        R_n = sigma ** 2 * np.eye(d)
    else:                                                    # :599-602
        T_H, r_n = H_X, r_o
        R_n = sigma ** 2 * np.eye(m)
    S = T_H @ P @ T_H.T + R_n                                # :605
    Kg = P @ T_H.T @ np.linalg.inv(S)                        # :606
    dx = Kg @ r_n                                            # :607
    I = np.eye(d)
    Pn = (I - Kg @ T_H) @ P @ (I - Kg @ T_H).T + Kg @ R_n @ Kg.T  # :613
    Pn = (Pn + Pn.T) / 2                                     # :614
    out.update(status=0, dx=dx, P_new=Pn)
    return out


# ---- the GPU cases (tests/test_gpu_view_sigma.py) ---------------------------------------------------------------------------
# name -> (N, F, M, make_problem's switches, engine plan); the smallest shapes that reach each k_feature form and K5 plan
SHAPES = {
    "one_chunk": (8, 24, 6, {}, "auto"),                                           # k_feature<24>, every track the same 6 views
    "band": (30, 120, 10, {"variable_tracks": True}, "auto"),                      # k_feature<24>, band pipeline, ragged
    # (plan "band": left to itself the engine splits this batch's 11 - 15-slot tracks -- 42 of 100 -- and no 90-column tile runs)
    "tiles90": (30, 100, 15, {"variable_tracks": True}, "band"),                   # k_feature<32>: two chunks; 90-column tiles
    "ring": (52, 100, 10, {}, "auto"),                                             # 60-column tiles, R in a ring
    "split": (20, 40, 20, {"variable_tracks": True, "min_track": 2}, "auto"),      # k_feature<64, true>: long tracks split
    "unsplit31": (31, 16, 31, {}, "band"),                                         # k_feature<64>: 31-view tracks as they are
}
# Seeds: the first seed from SEED_BASE + (index of the shape) for which, in every weighting the GPU tests use (none, uniform
# sigma / 2, the heterogeneous draw), the restatement updates (status 0) and no track's |gamma - crit| < 1e-6 crit: a gate
# decision within rounding of the threshold is no parity case.  Seeds that were skipped: SEED_SKIPS (shape -> seeds).
SEED_BASE = 9100
SEED_SKIPS = {}
HET_POWERS = (-1, 0, 1, 2)                                                         # sigma_v = sigma 2^k


def shape_seed(name):
    return SEED_BASE + list(SHAPES).index(name) + 100 * len(SEED_SKIPS.get(name, ()))


def make_shape(name):
    from msckf_amd import synth
    N, F, M, kw, _ = SHAPES[name]
    return synth.make_problem(N, F, M, seed=shape_seed(name), **kw)


def het_sigma(prob, seed):
    """sigma_v = sigma 2^k, k drawn per view from HET_POWERS."""
    rng = np.random.default_rng(seed)
    k = rng.choice(np.array(HET_POWERS), size=int(prob.view_ptr[-1]))
    return float(prob.sigma) * np.exp2(k.astype(np.float64))


def clear_of_threshold(out):
    return bool(np.all(np.abs(out["gamma"] - out["crit"]) >= 1e-6 * out["crit"]))
