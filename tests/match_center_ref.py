"""A NumPy restatement of the predicted centre of the match's search window (`csrc/match_center.h`; not in the
reference), the `Store` model whose window is centred by it, and the scenes the tests use.

The rule.  R_n, t_n: the pose of the newest clone; K: the intrinsics.  project(w): c = R_n^T w, h = K c, the centre
(h_x / h_z, h_y / h_z), defined iff h_z > 0 and both are finite.  ROTATED: w = d, the stored direction of the track's last
view.  POINT: w = rho (base - t_n) + m, defined only for a triangulated track with rho > 0.  Mode POINT takes ROTATED where
POINT is undefined; a track whose ROTATED centre is undefined has no centre (NaN, NaN).  how: 0 last keypoint, 1 rotated,
2 point, 3 none.  `centre(..., dtype=np.longdouble)` is the truth the tolerance of `test_match_center.py` is taken from."""
import numpy as np

import match_options_ref as mo
import match_ref

LAST, ROTATED, POINT = 0, 1, 2
HOW_LAST, HOW_ROTATED, HOW_POINT, HOW_NONE = 0, 1, 2, 3
MODES = {"last": LAST, "rotated": ROTATED, "point": POINT}
K = np.array([[400.0, 0.0, 320.0], [0.0, 400.0, 240.0], [0.0, 0.0, 1.0]])
WIDTH, HEIGHT = 640, 480
RADIUS = 12.0
GUARD_PX = mo.GUARD_PX
FAR = 1e9                                         # where `guards` puts a track without a centre to take distances from
BOUND_HZ, ANY_HZ, BOUND_LEVER = 0.2, 1e-3, 10.0   # h_z / |c| of a case the bound is taken from; |h_z| / |c| of any case; |rho (base - t_n)|


def project(Rn, Km, w):
    """project(w) in the dtype of its arguments, every product and sum written out as the header writes it; None: undefined."""
    c = [Rn[0, i] * w[0] + Rn[1, i] * w[1] + Rn[2, i] * w[2] for i in range(3)]
    h = [Km[i, 0] * c[0] + Km[i, 1] * c[1] + Km[i, 2] * c[2] for i in range(3)]
    if not h[2] > 0:
        return None
    with np.errstate(all="ignore"):
        u, v = h[0] / h[2], h[1] / h[2]
    if not (np.isfinite(u) and np.isfinite(v)):
        return None
    return u, v


def centre(mode, Rn, tn, Km, d, base, m, rho, tri, last_uv=None, dtype=np.float64):
    """((u, v), how) of one track, evaluated in `dtype`."""
    if mode == LAST:
        return (dtype(last_uv[0]), dtype(last_uv[1])), HOW_LAST
    Rn, Km = np.asarray(Rn, dtype=dtype).reshape(3, 3), np.asarray(Km, dtype=dtype).reshape(3, 3)
    tn, d, base, m = (np.asarray(x, dtype=dtype).reshape(3) for x in (tn, d, base, m))
    rho = dtype(rho)
    if mode == POINT and tri and rho > 0:
        p = project(Rn, Km, [rho * (base[k] - tn[k]) + m[k] for k in range(3)])
        if p is not None:
            return p, HOW_POINT
    p = project(Rn, Km, d)
    if p is not None:
        return p, HOW_ROTATED
    return (dtype(np.nan), dtype(np.nan)), HOW_NONE


def conditions(mode, Rn, tn, Km, d, base, m, rho, tri):
    """(fit for any test, fit for the bound) of one case, judged in long double: every projection the rule may evaluate has
    |h_z| >= ANY_HZ |c|; the one it takes has h_z >= BOUND_HZ |c| and, for POINT, |rho (base - t_n)| <= BOUND_LEVER."""
    L = np.longdouble
    Rn, Km = np.asarray(Rn, dtype=L).reshape(3, 3), np.asarray(Km, dtype=L).reshape(3, 3)
    tn, d, base, m = (np.asarray(x, dtype=L).reshape(3) for x in (tn, d, base, m))

    def ratio(w):
        c = Rn.T @ w
        return (Km @ c)[2] / np.sqrt(c @ c)
    lever = L(rho) * (base - tn)
    point = mode == POINT and tri and rho > 0
    ratios = [ratio(d)] + ([ratio(lever + m)] if point else [])
    fit = all(abs(r) >= ANY_HZ for r in ratios)
    taken = ratios[1] if point and ratios[1] > 0 else ratios[0]
    took_point = point and ratios[1] > 0
    bound = fit and taken >= BOUND_HZ and (not took_point or np.sqrt(lever @ lever) <= BOUND_LEVER)
    return fit, bool(bound)


# ---- the case set of the header driver and of the tolerance --------------------------------------------------------------
def _rotation(rng):
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    th = rng.uniform(-np.pi, np.pi)
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * (S @ S)


def _bearing(rng, kind):
    """A unit vector in the camera frame whose z (= h_z / |c| under a K with last row 0 0 1) is of the kind."""
    z = {"front": rng.uniform(BOUND_HZ + 0.01, 1.0), "grazing": rng.uniform(2 * ANY_HZ, BOUND_HZ - 0.01),
         "behind": -rng.uniform(2 * ANY_HZ, 1.0)}[kind]
    phi = rng.uniform(0, 2 * np.pi)
    s = np.sqrt(1 - z * z)
    return np.array([s * np.cos(phi), s * np.sin(phi), z])


def case_set(n=600, seed=7):
    """n cases as a dict of arrays (mode, tri int32; Rn (n, 9), tn, K (n, 9), d, base, m (n, 3), rho), every one fit for
    any test; `bound` marks those the tolerance is taken from.  Bearings and points in front, grazing and behind; both
    modes; triangulated or not; rho positive, zero and negative; a second K with skew and unequal focal lengths."""
    rng = np.random.default_rng(seed)
    K2 = np.array([[455.5, 0.7, 318.25], [0.0, 461.0, 243.5], [0.0, 0.0, 1.0]])
    out = {k: [] for k in ("mode", "tri", "Rn", "tn", "K", "d", "base", "m", "rho", "bound")}
    kinds = ("front", "front", "front", "grazing", "behind")
    while len(out["mode"]) < n:
        i = len(out["mode"])
        Rn, tn = _rotation(rng), rng.uniform(-2, 2, 3)
        Km = K if i % 3 else K2
        d = rng.uniform(0.5, 3.0) * (Rn @ _bearing(rng, kinds[i % 5]))
        W = tn + rng.uniform(2.0, 15.0) * (Rn @ _bearing(rng, kinds[(i // 5) % 5]))     # the point, by its bearing in the newest clone
        base = tn + rng.uniform(-1, 1, 3) * rng.uniform(0.0, 4.0)
        rho = 1.0 / np.linalg.norm(W - base)
        m = (W - base) * rho
        mode = ROTATED if i % 4 == 0 else POINT
        tri = int(i % 7 != 0)
        if i % 11 == 0:
            rho = 0.0 if i % 22 == 0 else -rho
        fit, bound = conditions(mode, Rn, tn, Km, d, base, m, rho, tri)
        if not fit:
            continue
        for k, v in (("mode", mode), ("tri", tri), ("Rn", Rn.reshape(9)), ("tn", tn), ("K", Km.reshape(9)), ("d", d), ("base", base),
                     ("m", m), ("rho", rho), ("bound", bound)):
            out[k].append(v)
    return {k: np.array(v, dtype=np.int32 if k in ("mode", "tri") else bool if k == "bound" else np.float64) for k, v in out.items()}


def evaluate(cs, dtype=np.float64):
    """(uv (n, 2) in dtype, how (n,)) of a case set."""
    n = len(cs["mode"])
    uv, how = np.zeros((n, 2), dtype=dtype), np.zeros(n, dtype=np.uint8)
    for i in range(n):
        uv[i], how[i] = centre(int(cs["mode"][i]), cs["Rn"][i], cs["tn"][i], cs["K"][i], cs["d"][i], cs["base"][i], cs["m"][i],
                               cs["rho"][i], bool(cs["tri"][i]), dtype=dtype)
    return uv, how


def pixel_error(got, truth):
    """The worst |got - truth| in pixels over the rows where the truth is a centre (NaN rows must be NaN in both)."""
    truth = np.asarray(truth)
    none = np.isnan(truth.astype(np.float64)).any(axis=1)
    assert np.array_equal(np.isnan(np.asarray(got, dtype=np.float64)).any(axis=1), none)
    if none.all():
        return 0.0
    return float(np.max(np.abs(np.asarray(got, dtype=truth.dtype)[~none] - truth[~none])))


# ---- the store whose window is centred by the rule ----------------------------------------------------------------------------
class Store(mo.Store):
    """`match_options_ref.Store` with the window centred under a mode.  `points`: id -> (base, m, rho) of the triangulated
    tracks (the caller keeps it: exact points, or what the engine's selection wrote back)."""

    def __init__(self, Km, min_cos, thr_e, thr_h, radius=0.0, margin=0.0, guarded=True, mode=LAST):
        super().__init__(Km, min_cos, thr_e, thr_h, radius, margin, guarded)
        self.mode = MODES.get(mode, mode)
        self.points = {}
        self.newest = None

    def add_camera(self, key, R, t):
        super().add_camera(key, R, t)
        self.newest = key

    def centres_how(self):
        Rn, tn = self.cams[self.newest]
        Kinv = np.linalg.inv(self.K)
        uv, how = [], []
        for t in self.table_ids:
            tr = self.tracks[t]
            u, v = tr.uv[-1]
            d = self.cams[tr.keys[-1]][0] @ (Kinv @ np.array([u, v, 1.0]))
            base, m, rho = self.points.get(t, (np.zeros(3), np.zeros(3), 0.0))
            c, h = centre(self.mode, Rn, tn, self.K, d, base, m, rho, t in self.points, last_uv=(u, v))
            uv.append(c), how.append(h)
        return np.array(uv, dtype=np.float64).reshape(-1, 2), np.array(how, dtype=np.uint8)

    def centres(self):
        """What the window's rule reads: NaN, NaN for a track without a centre."""
        return self.centres_how()[0]

    def intake(self, key, keypoints, descriptors, scores):
        kps = np.asarray(keypoints, dtype=np.float64).reshape(-1, 2)
        self.last = None

        def rule(A, B, min_cos):
            fn = guards if self.guarded else mo.match
            self.last = fn(A, B, min_cos, self.centres(), kps, self.radius, self.margin)
            return self.last.idx1, self.last.idx2, self.last.S

        plain, match_ref.match = match_ref.match, rule                # (match_ref.Store.intake looks the rule up in its module)
        try:
            return match_ref.Store.intake(self, key, keypoints, descriptors, scores)
        finally:
            match_ref.match = plain


def guards(A, B, min_cos, uv_table, uv_frame, radius=0.0, margin=0.0):
    """`match_options_ref.guards` for centres of which some are NaN.  The match is the rule's own with the NaN centres passed
    through `allowed()`, where `NaN <= r^2` is false as it is on the device: such a row meets no keypoint.  The guards cannot
    take a distance from NaN, so they are checked on a copy with those rows at a finite far point, which must decide every
    element alike; the rows without a centre have no distance to keep from the radius."""
    c = np.asarray(uv_table, dtype=np.float64).reshape(-1, 2)
    m = mo.match(A, B, min_cos, c, uv_frame, radius, margin)
    none = np.isnan(c).any(axis=1)
    if radius > 0:
        assert (m.why[none] == 1).all() and (m.m12[none] == mo.NONE).all()
    g = mo.guards(A, B, min_cos, np.where(none[:, None], FAR, c), uv_frame, radius, margin)
    for k in ("why", "m12", "m21", "idx1", "idx2"):
        assert np.array_equal(getattr(m, k), getattr(g, k)), k
    return m


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------
D = 64
MIN_COS = 0.8


def yaw(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def _sites():
    k = np.arange(mo.SITE_COLS * mo.SITE_ROWS)
    return np.column_stack([50.0 + mo.SITE_STEP * (k % mo.SITE_COLS), 30.0 + mo.SITE_STEP * (k // mo.SITE_COLS)])


def scene(poses, depth, seed):
    """The 10 x 8 grid of sites seen from `poses` [(R, t)]: a point per site at depth U(depth) in front of frame 0's camera.
    Returns a dict: W (80, 3); frames: per pose (who, kp, desc) -- the points whose projection is inside the image, in shuffled
    order, their keypoints and fp32 descriptors; proj: per pose the projection of every point (NaN behind the camera)."""
    rng = np.random.default_rng(seed)
    uv0 = _sites()
    R0, t0 = poses[0]
    z = rng.uniform(*depth, len(uv0))
    W = (np.linalg.inv(K) @ np.column_stack([uv0, np.ones(len(uv0))]).T * z).T @ R0.T + t0
    base = np.array([mo._unit(rng.standard_normal(D)) for _ in uv0])
    frames, proj = [], []
    for R, t in poses:
        c = (W - t) @ R
        with np.errstate(all="ignore"):
            p = (c @ K.T)[:, :2] / c[:, 2:3]
        p[c[:, 2] <= 0] = np.nan
        inside = (p[:, 0] >= 0) & (p[:, 0] < WIDTH) & (p[:, 1] >= 0) & (p[:, 1] < HEIGHT)
        who = rng.permutation(np.nonzero(inside)[0])
        d = base[who] * rng.uniform(0.95, 1.05, (len(who), 1)) + 0.02 * rng.standard_normal((len(who), D)) / np.sqrt(D)
        frames.append((who, p[who], d.astype(np.float32)))
        proj.append(p)
    return dict(W=W, frames=frames, proj=proj, poses=poses)


YAW_DEG, YAW_STEP, YAW_FRAMES = 4.0, 0.05, 6


def yaw_sweep(seed=3):
    """Frame 0 creates the tracks; six frames follow, each 4 degrees of yaw and 0.05 m further; depths 8-12 m."""
    poses = [(yaw(YAW_DEG * k), np.array([YAW_STEP * k, 0.0, 0.0])) for k in range(YAW_FRAMES + 1)]
    return scene(poses, (8.0, 12.0), seed)


LATERAL_STEP = 0.4


def lateral_step(seed=3):
    """Three frames, identity rotation, 0.4 m to the side per frame; depths 4-5 m."""
    poses = [(np.eye(3), np.array([LATERAL_STEP * k, 0.0, 0.0])) for k in range(3)]
    return scene(poses, (4.0, 5.0), seed)


def exact_point(W, anchor_t):
    """(base, m, rho) of the world point W anchored at the clone position anchor_t."""
    r = np.linalg.norm(W - anchor_t)
    return np.array(anchor_t, dtype=np.float64), (W - anchor_t) / r, 1.0 / r


def window_distances(centres, kp):
    """(T, n) distances between centres and keypoints (NaN centres: +inf)."""
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 1, 2)
    d = np.sqrt(((np.asarray(kp, dtype=np.float64).reshape(1, -1, 2) - c) ** 2).sum(axis=2))
    return np.where(np.isnan(d), np.inf, d)
