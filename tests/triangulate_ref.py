"""NumPy restatement of the device's refinement of triangulated points (k_select_refine), in fp64 and,
with `dtype=np.longdouble`, in extended precision.  Test infrastructure: nothing in the package imports it.

The algorithm, per track that the linear step flagged VALID | REFRESHED, anchor a = obs_slot[first view], CURRENT poses:
    x = (alpha, beta, rho);   h_i = R_s^T (R_a [alpha, beta, 1]^T + rho (t_a - t_s)),   zhat_i = h_xy / h_z
    z_i = K^-1 [u, v, 1] dehomogenised,   e_i = z_i - zhat_i,   c = sum_i w_i |e_i|^2,   w_i = line_conf[i]
    start x0 = (C_x / C_z, C_y / C_z, 1 / C_z), C = R_a^T (W_linear - t_a); attempted iff C_z > 0 and every h_z > 0 at x0
    Levenberg-Marquardt, lambda0 = 1e-3: (A + lambda diag A) d = g, A = sum w J^T J, g = sum w J^T e, 3x3 by cofactors
    a trial is accepted iff every h_z > 0, it is finite and its cost is strictly smaller:
        accept: lambda <- max(lambda / 10, 1e-12), stop when max|d| <= 1e-9 max(1, max|x|)   (x after the step)
        reject: lambda <- 10 lambda, stop when lambda > 1e8
    at most `iters` trials
    W = t_a + R_a [alpha, beta, 1]^T / rho is kept iff a trial was accepted, rho > 0 and W passes the anchor in-image
    test of the linear point; then world <- W, idp_m / idp_rho are refreshed from W the way the linear step does it
    (m = the unit bearing of the re-projected pixel, rho = 1 / depth in the anchor) and bit 8 is set.
Bits 1, 2 and 4 are never touched, and a track that is not kept stays exactly as the linear step left it.
"""
import numpy as np

FLAG_VALID, FLAG_LOST, FLAG_REFRESHED, FLAG_REFINED = 1, 2, 4, 8
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, STEP_TOL = 1e-3, 1e-12, 1e8, 1e-9


def lane_sum(terms):
    """Sum over the views (axis 0) in the kernel's order: lane `sub` of the track's eight adds its views sub, sub + 8,
    ... one after the other, then the DPP tree ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7))."""
    M = terms.shape[0]
    pad = np.zeros(((-M) % 8,) + terms.shape[1:], dtype=terms.dtype)
    rounds = np.concatenate([terms, pad]).reshape((-1, 8) + terms.shape[1:])
    lane = rounds[0]
    for r in rounds[1:]:
        lane = lane + r
    return ((lane[0] + lane[1]) + (lane[2] + lane[3])) + ((lane[4] + lane[5]) + (lane[6] + lane[7]))


def normal_equations(x, Ra, ta, Rs, ts, z, w):
    """A (3, 3), g (3,), the cost and `feasible` (every h_z > 0) at x, all in x's dtype.  Rs (M, 3, 3), ts (M, 3): the
    poses of the views' clones; z (M, 2) the normalised observations; w (M,).  Every expression is written in the
    kernel's order of operations (which is compiled without contraction into fused multiply-adds), so that in fp64 the
    two take the same decisions at the same trials."""
    al, be, rho = x
    r = Ra[:, 0] * al + Ra[:, 1] * be + Ra[:, 2]                  # the anchor's ray R_a [alpha, beta, 1]
    d = ta[None, :] - ts
    y = r[None, :] + rho * d
    RT = lambda v: Rs[:, 0, :] * v[:, 0:1] + Rs[:, 1, :] * v[:, 1:2] + Rs[:, 2, :] * v[:, 2:3]      # R_s^T v, per view
    h = RT(y)
    p = [RT(np.broadcast_to(Ra[:, 0], d.shape)), RT(np.broadcast_to(Ra[:, 1], d.shape)), RT(d)]
    hz = h[:, 2]
    feasible = bool(np.all(hz > 0))
    with np.errstate(all="ignore"):
        zh0, zh1 = h[:, 0] / hz, h[:, 1] / hz
        e0, e1 = z[:, 0] - zh0, z[:, 1] - zh1
        j0 = [(q[:, 0] - zh0 * q[:, 2]) / hz for q in p]
        j1 = [(q[:, 1] - zh1 * q[:, 2]) / hz for q in p]
        A = np.zeros((3, 3), dtype=x.dtype)
        for k in range(3):
            for l in range(k, 3):
                A[k, l] = A[l, k] = lane_sum(w * (j0[k] * j0[l] + j1[k] * j1[l]))
        g = np.array([lane_sum(w * (j0[k] * e0 + j1[k] * e1)) for k in range(3)], dtype=x.dtype)
        c = lane_sum(w * (e0 * e0 + e1 * e1))
    return A, g, c, feasible


def solve_damped(A, g, lam):
    """(A + lam diag A) d = g by cofactors."""
    m00, m11, m22 = A[0, 0] + lam * A[0, 0], A[1, 1] + lam * A[1, 1], A[2, 2] + lam * A[2, 2]
    m01, m02, m12 = A[0, 1], A[0, 2], A[1, 2]
    k00, k01, k02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
    k11, k12, k22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
    with np.errstate(all="ignore"):
        det = m00 * k00 + m01 * k01 + m02 * k02
        return np.array([(k00 * g[0] + k01 * g[1] + k02 * g[2]) / det,
                         (k01 * g[0] + k11 * g[1] + k12 * g[2]) / det,
                         (k02 * g[0] + k12 * g[1] + k22 * g[2]) / det], dtype=A.dtype)


def normalised(uv, Kinv):
    """z = K^-1 [u, v, 1] dehomogenised, (M, 2)."""
    u, v = uv[:, 0], uv[:, 1]
    zx, zy, zw = (Kinv[i, 0] * u + Kinv[i, 1] * v + Kinv[i, 2] for i in range(3))
    return np.stack([zx / zw, zy / zw], axis=1)


def anchor_refresh(W, Ra, ta, K, Kinv, width, height):
    """The anchor in-image test of the linear step and the refreshed (m, rho); None when W fails the test."""
    C = Ra.T @ (W - ta)
    if not C[2] > 0:
        return None
    im = K @ C
    u, v = im[0] / im[2], im[1] / im[2]
    if u < 0 or u >= width or v < 0 or v >= height:
        return None
    Wv = Ra @ (Kinv @ np.array([u, v, 1.0], dtype=W.dtype))
    return Wv / np.sqrt(np.sum(Wv * Wv)), 1.0 / C[2]


def refine_track(W_lin, Ra, ta, Rs, ts, uv, w, K, width, height, iters, dtype=np.float64):
    """One track.  Returns a dict: attempted, kept, x (alpha, beta, rho), world, idp (m, rho) or None, cost0, cost1, trials."""
    T = lambda a: np.asarray(a, dtype=dtype)
    Ra, ta, Rs, ts, w, K, W_lin = T(Ra), T(ta), T(Rs), T(ts), T(w), T(K), T(W_lin)
    # K^-1 of an upper-triangular pinhole matrix in the working precision (np.linalg.inv has no long double)
    Kinv = T(np.linalg.inv(np.asarray(K, dtype=np.float64)))
    if dtype is not np.float64:
        Kinv = Kinv + Kinv @ (np.eye(3, dtype=dtype) - K @ Kinv)      # one Newton step: exact to the working precision
    z = normalised(T(uv), Kinv)
    out = dict(attempted=False, kept=False, x=np.full(3, np.nan), world=W_lin, idp=None, cost0=0.0, cost1=0.0, trials=0)
    q = W_lin - ta
    C = Ra[0, :] * q[0] + Ra[1, :] * q[1] + Ra[2, :] * q[2]          # R_a^T (W - t_a)
    if not C[2] > 0:
        return out
    x = np.array([C[0] / C[2], C[1] / C[2], 1.0 / C[2]], dtype=dtype)
    A, g, c, feasible = normal_equations(x, Ra, ta, Rs, ts, z, w)
    out["x"] = x
    if not feasible:
        return out
    out.update(attempted=True, cost0=c, cost1=c)
    lam, moved, trials = dtype(LAMBDA0), False, 0
    for _ in range(int(iters)):
        d = solve_damped(A, g, lam)
        xt = x + d
        At, gt, ct, ok = normal_equations(xt, Ra, ta, Rs, ts, z, w)
        trials += 1
        if ok and np.all(np.isfinite(xt)) and np.isfinite(ct) and ct < c:
            x, A, g, c, moved = xt, At, gt, ct, True
            lam = max(lam / 10.0, dtype(LAMBDA_MIN))
            if np.max(np.abs(d)) <= STEP_TOL * max(1.0, np.max(np.abs(x))):
                break
        else:
            lam = lam * 10.0
            if lam > LAMBDA_MAX:
                break
    out.update(x=x, trials=trials)
    if moved and x[2] > 0:
        W = ta + (Ra[:, 0] * x[0] + Ra[:, 1] * x[1] + Ra[:, 2]) / x[2]
        idp = anchor_refresh(W, Ra, ta, K, Kinv, width, height)
        if idp is not None:
            out.update(kept=True, world=W, idp=idp, cost1=c)
    return out


def track_views(prob, tracks, j):
    """What the refinement reads of track j: anchor pose, the views' poses, pixels, weights."""
    a, b = int(prob.view_ptr[j]), int(prob.view_ptr[j + 1])
    slots = np.asarray(prob.obs_slot[a:b], dtype=np.int64)
    return (prob.cam_R[slots[0]], prob.cam_t[slots[0]], prob.cam_R[slots], prob.cam_t[slots],
            np.asarray(prob.obs_uv, dtype=np.float64).reshape(-1, 2)[a:b], np.asarray(tracks.line_conf, dtype=np.float64)[a:b])


def refine_batch(prob, tracks, params, linear, iters, dtype=np.float64):
    """The refinement pass over a batch.  `linear`: the result of the linear step (`oracle.select_features`, or the
    device's own unrefined selection as a dict) with `flags`, `world`, `idp_m`, `idp_rho`.  Returns the same four as
    they stand afterwards (fp64), plus `x` (F, 3; NaN where no start was formed), `attempted`, `kept`, `cost0`, `cost1`
    (in `dtype`) and `trials`."""
    F = prob.F
    flags = np.array(linear["flags"], dtype=np.uint8)
    world, idp_m, idp_rho = np.array(linear["world"]), np.array(linear["idp_m"]), np.array(linear["idp_rho"])
    x = np.full((F, 3), np.nan, dtype=dtype)
    world_hi = np.array(world, dtype=dtype)
    cost0, cost1 = np.zeros(F, dtype=dtype), np.zeros(F, dtype=dtype)
    trials = np.zeros(F, dtype=np.int32)
    attempted, kept = np.zeros(F, dtype=bool), np.zeros(F, dtype=bool)
    want = FLAG_VALID | FLAG_REFRESHED
    for j in range(F):
        if (flags[j] & want) != want:
            continue
        Ra, ta, Rs, ts, uv, w = track_views(prob, tracks, j)
        r = refine_track(linear["world"][j], Ra, ta, Rs, ts, uv, w, prob.K, params.width, params.height, iters, dtype)
        attempted[j], kept[j], trials[j] = r["attempted"], r["kept"], r["trials"] if r["attempted"] else 0
        x[j] = r["x"]
        if r["attempted"]:
            cost0[j], cost1[j] = r["cost0"], r["cost1"]
        if r["kept"]:
            flags[j] |= FLAG_REFINED
            world_hi[j] = r["world"]
            world[j] = r["world"].astype(np.float64)
            idp_m[j], idp_rho[j] = r["idp"][0].astype(np.float64), float(r["idp"][1])
    return dict(flags=flags, world=world, world_hi=world_hi, idp_m=idp_m, idp_rho=idp_rho, x=x, attempted=attempted,
                kept=kept, cost0=cost0, cost1=cost1, trials=trials)


def cost_at_world(prob, tracks, j, W):
    """The weighted reprojection cost of track j at the world point W under the batch's poses (fp64):
    h_i = R_s^T (W - t_s), which is the model's h_i / rho."""
    _, _, Rs, ts, uv, w = track_views(prob, tracks, j)
    Kinv = np.linalg.inv(np.asarray(prob.K, dtype=np.float64))
    z = normalised(uv, Kinv)
    h = np.einsum("mji,mj->mi", Rs, np.asarray(W, dtype=np.float64)[None, :] - ts)
    e = z - h[:, :2] / h[:, 2:3]
    return float(np.sum(w * np.sum(e * e, axis=1)))


def rel_spread(a, b):
    """Per-track relative distance of two (F, k) arrays: max|a - b| / max(1, max|b|) over the k entries."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return (np.max(np.abs(a - b), axis=1) / np.maximum(1.0, np.max(np.abs(b), axis=1))).astype(np.float64)
