"""A NumPy restatement of the match behind its two options (not in the reference; `include/msckf_mi355x.h`): a
search window around each track's last stored keypoint and a margin between the best and the second-best similarity.

The rule.  A: the table, T x D, rows in creation order; B: the frame, n x D; S = A B^T (`match_ref.similarity`).
allowed(i, j): the radius is off (0), or (u_j - u^_i)^2 + (v_j - v^_i)^2 <= radius^2 in double, (u^_i, v^_i) the last stored
keypoint of table track i.  S'[i, j] = S[i, j] where allowed, else -inf.  m12[i] = argmax_j S'[i, .], lowest index among
equals, or none (-1) when no j is allowed; s1 that maximum; s2 the largest S'[i, j] over j != m12[i], -inf when there is
none.  The same per column: m21, c1, c2.  Each table element gets a reason code, the first that applies:
  1  no keypoint inside the window
  2  m21[m12[i]] != i
  3  not s1 > min_cos (strict)
  4  the margin is on (> 0) and not (s1 - s2 > margin and c1 - c2 > margin), c1 / c2 of column m12[i]; -inf passes
  0  the pair (i, m12[i])
With radius = +inf and margin = 0 this is `match_ref.match`.

`scene()` builds the frames the tests use: tracks on a grid of sites further apart than the window, re-observed, lost, met by
strangers, and 'twins' -- pairs of tracks with near-equal descriptors, far apart (the aliasing the window removes) or inside
one another's window (where mutuality and the margin decide)."""
from types import SimpleNamespace

import numpy as np

import match_ref

GUARD = match_ref.GUARD
GUARD_PX = 1e-6
NONE = -1


def _best_two(M):
    """Per row of M (with -inf for what is masked): (argmax or NONE, best, second best over the other columns)."""
    rows, cols = M.shape
    arg = np.full(rows, NONE, dtype=np.int64)
    first = np.full(rows, -np.inf)
    second = np.full(rows, -np.inf)
    if cols == 0:
        return arg, first, second
    k = np.argmax(M, axis=1)                                         # the first of equal maxima
    first = M[np.arange(rows), k]
    some = first > -np.inf
    arg[some] = k[some]
    rest = M.copy()
    rest[np.arange(rows), k] = -np.inf
    second = rest.max(axis=1)
    return arg, first, second


def allowed(uv_table, uv_frame, radius, T, n):
    if not radius > 0:
        return np.ones((T, n), dtype=bool), None
    a = np.asarray(uv_table, dtype=np.float64).reshape(T, 2)
    b = np.asarray(uv_frame, dtype=np.float64).reshape(n, 2)
    du, dv = b[None, :, 0] - a[:, None, 0], b[None, :, 1] - a[:, None, 1]
    d2 = du * du + dv * dv
    return d2 <= float(radius) * float(radius), d2


def match(A, B, min_cos, uv_table=None, uv_frame=None, radius=0.0, margin=0.0):
    """The rule.  Returns a namespace: idx1, idx2 (the pairs, table rows ascending), why (T,), S, Sm (= S'), m12, s1, s2,
    m21, c1, c2, d2 (squared keypoint distances, None without a window)."""
    S = match_ref.similarity(A, B)
    T, n = S.shape
    ok, d2 = allowed(uv_table, uv_frame, radius, T, n)
    Sm = np.where(ok, S, -np.inf)
    m12, s1, s2 = _best_two(Sm)
    m21, c1, c2 = _best_two(Sm.T)
    why = np.zeros(T, dtype=np.uint8)
    for i in range(T):
        j = m12[i]
        if j == NONE:
            why[i] = 1
        elif m21[j] != i:
            why[i] = 2
        elif not s1[i] > min_cos:
            why[i] = 3
        elif margin > 0 and not (s1[i] - s2[i] > margin and c1[j] - c2[j] > margin):
            why[i] = 4
    idx1 = np.nonzero(why == 0)[0]
    return SimpleNamespace(idx1=idx1, idx2=m12[idx1], why=why, S=S, Sm=Sm, m12=m12, s1=s1, s2=s2, m21=m21, c1=c1, c2=c2, d2=d2)


def guards(A, B, min_cos, uv_table=None, uv_frame=None, radius=0.0, margin=0.0):
    """Raises AssertionError unless differently rounded fp32 sums cannot change a verdict: every best GUARD from its
    runner-up (both directions, among the allowed candidates) and from the threshold, every s1 - s2 and c1 - c2 GUARD from
    the margin, every keypoint distance GUARD_PX from the radius.  Returns the match."""
    m = match(A, B, min_cos, uv_table, uv_frame, radius, margin)
    for best, second in ((m.s1, m.s2), (m.c1, m.c2)):
        both = second > -np.inf
        if both.any():
            gap = float((best[both] - second[both]).min())
            assert gap >= GUARD, ("runner-up", gap)
            if margin > 0:
                off = float(np.abs(best[both] - second[both] - margin).min())
                assert off >= GUARD, ("margin", off)
        some = best > -np.inf
        if some.any():
            assert float(np.abs(best[some] - min_cos).min()) >= GUARD, "threshold"
    if m.d2 is not None and np.isfinite(radius) and m.d2.size:
        off = float(np.abs(np.sqrt(m.d2) - radius).min())
        assert off >= GUARD_PX, ("radius", off)
    return m


class Store(match_ref.Store):
    """`match_ref.Store` whose intake matches by the rule above, the window centred on each table track's last keypoint."""

    def __init__(self, K, min_cos, thr_e, thr_h, radius=0.0, margin=0.0, guarded=True):
        super().__init__(K, min_cos, thr_e, thr_h)
        self.radius, self.margin, self.guarded = float(radius), float(margin), guarded
        self.last = None                  # the last match (the namespace of `match`), None where none ran

    def centres(self):
        return np.array([self.tracks[t].uv[-1] for t in self.table_ids], dtype=np.float64).reshape(-1, 2)

    def intake(self, key, keypoints, descriptors, scores):
        kps = np.asarray(keypoints, dtype=np.float64).reshape(-1, 2)
        self.last = None

        def rule(A, B, min_cos):
            fn = guards if self.guarded else match
            self.last = fn(A, B, min_cos, self.centres(), kps, self.radius, self.margin)
            return self.last.idx1, self.last.idx2, self.last.S

        plain, match_ref.match = match_ref.match, rule                # (Store.intake looks the rule up in its module)
        try:
            return super().intake(key, keypoints, descriptors, scores)
        finally:
            match_ref.match = plain


# ---- the case set --------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 8), (15, 16, 8), (16, 17, 64), (17, 40, 64), (33, 16, 8), (48, 48, 64)]
MIN_COS, RADIUS, MARGIN = 0.8, 20.0, 0.05
MODES = {"window": (RADIUS, 0.0), "margin": (0.0, MARGIN), "both": (RADIUS, MARGIN)}
TWIN = 0.15                               # a twin's descriptor is unit(a + TWIN p), p a unit vector orthogonal to a
SITE_STEP, SITE_COLS, SITE_ROWS = 60.0, 10, 8


def _unit(v):
    return v / np.linalg.norm(v)


def _twin(rng, a):
    p = rng.standard_normal(len(a))
    p = _unit(p - (p @ a) * a)
    return _unit(a + TWIN * p)


def _plan(T, n):
    """How many groups of each kind a (T, n) scene holds: far twins (2 tracks, 2 keypoints, 2 sites), near twins both seen
    (2, 2, 1 site), near twins with one keypoint (2, 1), a track met by a stranger (1, 1), tracks seen (1, 1) and lost
    (1, 0), strangers on sites of their own (0, 1)."""
    if T < 8:
        seen = min(T, n)
        return dict(far=0, both=0, one=0, met=0, seen=seen, lost=T - seen, strangers=n - seen)
    far = min(T // 5, n // 3)
    k = 2 if T >= 40 else 1
    t, m = T - 2 * far - 5 * k, n - 2 * far - 4 * k
    lost = max(2, t - m)
    return dict(far=far, both=k, one=k, met=k, seen=t - lost, lost=lost, strangers=m - (t - lost))


def scene(T, n, D, seed):
    """One case: a dict with A (T, D) fp32, uvA (T, 2), B (n, D) fp32, uvB (n, 2), true (the (track, keypoint) pairs that are
    re-observations) -- tracks and keypoints in shuffled order."""
    rng = np.random.default_rng(seed)
    plan = _plan(T, n)
    sites = rng.permutation(SITE_COLS * SITE_ROWS)
    centre = np.column_stack([50.0 + SITE_STEP * (sites % SITE_COLS), 30.0 + SITE_STEP * (sites // SITE_COLS)])
    A, uvA, B, uvB, true = [], [], [], [], []
    site = iter(range(len(sites)))

    def track(s, a):
        A.append(a)
        uvA.append(centre[s] + rng.uniform(-3, 3, 2))
        return len(A) - 1

    def keypoint(b, at):
        B.append(b)
        uvB.append(at + rng.uniform(-3, 3, 2))
        return len(B) - 1

    def fresh():
        return _unit(rng.standard_normal(D))

    for g in range(plan["far"]):
        a = fresh()
        a2 = _twin(rng, a)
        i, i2 = track(next(site), a), track(next(site), a2)
        s = rng.uniform(0.95, 1.05)
        if g % 2 == 0:                    # each is seen as the other's descriptor: the plain rule pairs them crosswise
            j, j2 = keypoint(s * a2, uvA[i]), keypoint(s * a, uvA[i2])
        else:                             # the second twin's keypoint is the louder one: it takes both rows' argmax
            j, j2 = keypoint(0.95 * a, uvA[i]), keypoint(1.1 * a2, uvA[i2])
        true += [(i, j), (i2, j2)]
    for _ in range(plan["both"]):         # inside one window, both seen: mutual, and a gap of s (1 - a . a2) ~ 0.011
        a, s, st = fresh(), rng.uniform(0.95, 1.05), next(site)
        a2 = _twin(rng, a)
        i, i2 = track(st, a), track(st, a2)
        true += [(i, keypoint(s * a, uvA[i])), (i2, keypoint(s * a2, uvA[i2]))]
    for _ in range(plan["one"]):          # inside one window, one keypoint: the second twin is not mutual
        a, s, st = fresh(), rng.uniform(0.95, 1.05), next(site)
        i = track(st, a)
        track(st, _twin(rng, a))
        true.append((i, keypoint(s * a, uvA[i])))
    for _ in range(plan["met"]):          # a stranger inside the window: mutual, below the threshold
        a = fresh()
        i = track(next(site), a)
        b = fresh()
        keypoint(_unit(b - (b @ a) * a) * 0.9 + 0.3 * a, uvA[i])
    for _ in range(plan["seen"]):
        a = fresh()
        i = track(next(site), a)
        true.append((i, keypoint(rng.uniform(0.95, 1.1) * a + 0.03 * rng.standard_normal(D) / np.sqrt(D), uvA[i])))
    for _ in range(plan["lost"]):
        track(next(site), fresh())
    for _ in range(plan["strangers"]):
        keypoint(fresh() * rng.uniform(0.9, 1.1), centre[next(site)])
    assert len(A) == T and len(B) == n, (len(A), len(B), plan)
    pt, pk = rng.permutation(T), rng.permutation(n)                   # position -> original index
    it, ik = np.argsort(pt), np.argsort(pk)
    return dict(A=np.asarray(A, dtype=np.float32)[pt], uvA=np.asarray(uvA)[pt], B=np.asarray(B, dtype=np.float32)[pk],
                uvB=np.asarray(uvB)[pk], true=sorted((int(it[i]), int(ik[j])) for i, j in true), plan=plan, seed=seed)


def case(T, n, D):
    """The scene of one shape from its first seed that passes `guards()` under every mode and under the plain rule."""
    for seed in range(100 * T + n, 100 * T + n + 50):
        c = scene(T, n, D, seed)
        try:
            match_ref.guards(c["A"], c["B"], MIN_COS, need_pairs=False)
            for radius, margin in MODES.values():
                guards(c["A"], c["B"], MIN_COS, c["uvA"], c["uvB"], radius, margin)
        except AssertionError:
            continue
        return c
    raise AssertionError("no seed met the guards")


def score(c, idx1, idx2):
    """(true pairs found, wrong pairs) of a match on a scene."""
    true = set(c["true"])
    got = set(zip(np.asarray(idx1).tolist(), np.asarray(idx2).tolist()))
    return len(got & true), len(got - true)
