"""The batches of tests/test_wide_coverage.py (CPU) and tests/test_gpu_wide_coverage.py: what tests/wide_cases.py leaves open on
`k_feature_wide` (csrc/k_feature_wide.h), the second pass of `k_gather` and the 64-view slot map of `k_fold` / `k_fold_g`.

  A  lengths     one track of every length 32 .. 64 on a 64-clone window (`all_lengths`), and of the lengths at which 2M - 2 fills
                 whole 16-row strips under pure rotation (`all_lengths_rank2`): every tail of the kernel depends on M
  B  layouts     views that skip clones, tracks far from slot 0, views in a random order, windows of 65, 100 and 221 clones with
                 slots of 128 and above (`holes_64`, `shuffled`, `beyond_64`); batches that must be refused
  C  geometry    the families of tests/geometry_cases.py on a form of 32 .. 48 views (`wide`): K2's six pivot orders, rank 2,
                 pz < 0, a second K, off-clone anchors, rotated axes with a distinct null state

Every batch is built from full-length tracks of `geometry_cases.make_geometry` by `keep_views`, which keeps a chosen subset of
each track's views in a chosen order.  Host only, NumPy; not a conftest: imported by name.  Oracle results are computed once per
batch and shared: leave them unchanged."""
import functools
from collections import namedtuple

import numpy as np

import geometry_cases as gc
import wide_cases as wc
from msckf_amd import synth
from oracle import msckf_oracle as oracle

WIDE_TO = 64                      # MSCKF_MAX_TRACK_WIDE
LENGTHS = tuple(range(wc.WIDE_FROM, WIDE_TO + 1))
# pure rotation: q = 2M - 2.  M = 33, 49, 57 give q = 64, 96, 112 (a full last 16-row strip), M = 64 gives 126
RANK2_FULL_STRIPS = {33: 64, 49: 96, 57: 112, 64: 126}
RANK2_LENGTHS = tuple(sorted(set(range(32, 65, 2)) | {33, 63} | set(RANK2_FULL_STRIPS)))


def keep_views(prob, keep):
    """`prob` with track j's views `keep[j]` (positions in the track, in the order given) and no others."""
    idx, vp = [], [0]
    for j, k in enumerate(keep):
        a, M = int(prob.view_ptr[j]), int(prob.view_ptr[j + 1] - prob.view_ptr[j])
        k = [int(x) for x in k]
        assert len(k) and len(set(k)) == len(k) and min(k) >= 0 and max(k) < M, (j, k)
        idx += [a + x for x in k]
        vp.append(vp[-1] + len(k))
    idx = np.asarray(idx, dtype=np.int64)
    vs = None if prob.view_sigma is None else np.asarray(prob.view_sigma, dtype=np.float64).reshape(-1)[idx]
    return synth.UpdateProblem(**{**prob.__dict__, "view_ptr": np.asarray(vp, dtype=np.int32), "obs_uv": prob.obs_uv[idx],
                                  "obs_slot": prob.obs_slot[idx].astype(np.int32), "view_sigma": vs, "meta": dict(prob.meta, keep=keep)})


def track_slots(prob, j):
    return np.asarray(prob.obs_slot[prob.view_ptr[j]:prob.view_ptr[j + 1]])


def _update(prob):
    return oracle.update(prob, dense_noise=False)


# ---- A: every length -------------------------------------------------------------------------------------------------------------

# Seeds: the first of base, base + 1, ... at which the oracle alone meets the conditions of tests/test_wide_coverage.py
# (status 0, both verdicts among the wide tracks, gate margin >= wide_cases.MIN_MARGIN).  Every batch whose seed is not its base:
SEED_SKIPS = {"beyond_100": 1}             # seed 7500: the oracle accepts all four wide tracks
_BASE_SEED = {"all_lengths": 7100, "all_lengths_rank2": 7200, "holes_64": 7300, "beyond_65": 7400, "beyond_100": 7500, "beyond_221": 7600}


def seed_of(name):
    return _BASE_SEED[name] + SEED_SKIPS.get(name, 0)


def _full_tracks(N, F, seed, poses=None, gravity=None, **opts):
    """F tracks that see every clone of an N-clone corridor (or of `poses`): the stock `keep_views` cuts from.  The corridor
    advances 0.15 m per clone, so the points lie deeper than the window is long."""
    rng = np.random.default_rng([17, seed])
    if poses is None:
        poses = gc.corridor(N, rng)
    args = {**gc._GATE, "views": (N, N), "full_tracks": F, "depth": (0.15 * N + 6.0, 0.15 * N + 40.0), "lateral_extent": 0.25, "gravity": gravity}
    args.update(opts)
    return gc.make_geometry(poses, F, seed, **args)


def _consecutive(rng, lengths, N):
    keep = []
    for M in lengths:
        s0 = int(rng.integers(0, N - M + 1))
        keep.append(list(range(s0, s0 + M)))
    return keep


@functools.lru_cache(maxsize=None)
def all_lengths():
    """(prob, oracle.update): one track of each length 32 .. 64, consecutive views, a view 400 px off on a quarter of them."""
    seed = seed_of("all_lengths")
    base = _full_tracks(WIDE_TO, len(LENGTHS), seed, outlier_fraction=0.25)
    prob = keep_views(base, _consecutive(np.random.default_rng([19, seed]), LENGTHS, WIDE_TO))
    return prob, _update(prob)


@functools.lru_cache(maxsize=None)
def all_lengths_rank2():
    """(prob, oracle.update): RANK2_LENGTHS under pure rotation (wide_cases.rank2_case's recipe): rank 2 on every track."""
    seed = seed_of("all_lengths_rank2")
    rng = np.random.default_rng([11, seed])
    g = synth.GRAVITY_DEFAULT.copy()
    poses, g = gc.rotated_world(gc.pure_rotation(WIDE_TO, rng, rate=wc.ROTATION_RATE), g, gc.yaw(rng.uniform(0.0, 2.0 * np.pi)))
    base = _full_tracks(WIDE_TO, len(RANK2_LENGTHS), seed, poses=poses, gravity=g,
                        **{**gc._OPTIONS["rotation"], "horizon_fraction": 0.0, "outlier_fraction": 0.25})
    prob = keep_views(base, _consecutive(np.random.default_rng([19, seed]), RANK2_LENGTHS, WIDE_TO))
    return prob, _update(prob)


# ---- B: slot layouts -------------------------------------------------------------------------------------------------------------

def _subset(rng, M, lo, hi):
    """M of the slots lo .. hi - 1, ascending, the ends included."""
    inner = rng.choice(np.arange(lo + 1, hi - 1), size=M - 2, replace=False)
    return sorted([lo, hi - 1] + inner.tolist())


# holes_64: (what, views).  The first seven are wide; every track is cut from one that sees all 64 clones
def _holes_64_keep(rng):
    keep = [_subset(rng, M, 0, 64) for M in (32, 33, 40, 47, 63)]
    keep.append(list(range(0, 64, 2)))                          # the even slots
    keep.append(list(range(32, 64)))                            # far from slot 0
    keep.append([5, 60])                                        # narrow: two views 55 slots apart
    keep.append(_subset(rng, 10, 20, 50))
    keep.append(list(range(30, 40)))
    keep.append(_subset(rng, 31, 1, 64))
    return keep


HOLES_64_WIDE = (32, 33, 40, 47, 63, 32, 32)
HOLES_64_NARROW = (2, 10, 10, 31)


@functools.lru_cache(maxsize=None)
def holes_64():
    seed = seed_of("holes_64")
    base = _full_tracks(64, len(HOLES_64_WIDE) + len(HOLES_64_NARROW), seed)
    prob = keep_views(base, _holes_64_keep(np.random.default_rng([23, seed])))
    return prob, _update(prob)


def shuffled_tracks(prob):
    """Every second wide track of `prob`."""
    return np.nonzero(wc.wide(prob))[0][::2]


@functools.lru_cache(maxsize=None)
def shuffled():
    """holes_64 with every second wide track's views in a seeded random order, neither ascending nor descending.
    (prob, oracle.update of THIS order)."""
    prob, _ = holes_64()
    rng = np.random.default_rng([29, seed_of("holes_64")])
    keep = [list(range(int(m))) for m in wc.views(prob)]
    for j in shuffled_tracks(prob):
        k = rng.permutation(len(keep[j])).tolist()
        # the lowest slot (view 0 of the ascending track) goes among the views from 32 on, which k_gather takes in its second pass;
        # a track of 32 views has none: there it only leaves the front
        at, to = k.index(0), (len(k) - 1 if len(k) > 32 else 5)
        if at < 32 and len(k) > 32 or at == 0:
            k[at], k[to] = k[to], k[at]
        keep[j] = k
    out = keep_views(prob, keep)
    return out, _update(out)


# beyond_64: N -> ((views, lowest slot, one past the highest slot) of every track); the wide ones first
BEYOND = {
    65: ((64, 0, 65), (48, 3, 65), (33, 0, 60), (32, 30, 65), (2, 0, 65), (12, 40, 65), (31, 2, 64)),
    100: ((64, 0, 100), (48, 10, 95), (33, 64, 100), (32, 0, 70), (3, 0, 100), (9, 60, 100), (31, 20, 99)),
    221: ((64, 0, 221), (32, 128, 221), (48, 40, 200), (2, 0, 221), (20, 130, 221), (31, 100, 180)),
}
# the lowest slot a window of N clones can keep a whole wide track above: 128 where the window has 32 slots beyond it
HIGH_SLOT = {65: None, 100: 64, 221: 128}


@functools.lru_cache(maxsize=None)
def beyond_64(N):
    seed = seed_of(f"beyond_{N}")
    spec = BEYOND[N]
    base = _full_tracks(N, len(spec), seed)
    rng = np.random.default_rng([31, seed])
    prob = keep_views(base, [_subset(rng, M, lo, hi) for M, lo, hi in spec])
    return prob, _update(prob)


def with_duplicate_slot(prob, j, v_from, v_to):
    """`prob` with view v_to of track j on the clone of its view v_from."""
    sl = prob.obs_slot.copy()
    a = int(prob.view_ptr[j])
    sl[a + v_to] = sl[a + v_from]
    return synth.UpdateProblem(**{**prob.__dict__, "obs_slot": sl})


def with_slot(prob, j, v, slot):
    sl = prob.obs_slot.copy()
    sl[int(prob.view_ptr[j]) + v] = slot
    return synth.UpdateProblem(**{**prob.__dict__, "obs_slot": sl})


def layout_batches():
    """name -> (prob, ref) of every batch of B that is held against the oracle."""
    out = {"holes_64": holes_64(), "shuffled": shuffled()}
    for N in BEYOND:
        out[f"beyond_{N}"] = beyond_64(N)
    return out


# ---- C: geometry families at wide lengths ----------------------------------------------------------------------------------------

WIDE_FORM = (48, 16, (32, 48), False)             # (N, F, (shortest, longest track), views reversed), as geometry_cases.FORMS
FAMILIES = ("rotated", "lateral", "arc", "behind", "rotation", "still", "far", "anchor", "fx1400")
BEHIND_STEP = 0.03                                # lateral motion per clone of family "behind": 48 clones pass 1.4 m beside the points
# Seeds: 5000 + 10 x (position of the family) + k, with the first k at which the case meets every condition of
# tests/test_wide_coverage.py.  Every case whose k is not 0:
GEOMETRY_SEED_SKIPS = {}

WideCase = namedtuple("WideCase", "name family seed exact_rank2")


def _wide_cases():
    out = {}
    for fi, family in enumerate(FAMILIES):
        name = f"{family}_wide"
        out[name] = WideCase(name, family, 5000 + 10 * fi + GEOMETRY_SEED_SKIPS.get(name, 0), family in gc.EXACT_RANK2)
    return out


GEOMETRY = _wide_cases()


def _wide_poses(family, N, rng):
    g = synth.GRAVITY_DEFAULT.copy()
    if family == "behind":                        # (on geometry_cases' arc no track of 32 views keeps a view with pz < 0 in the image)
        return gc.lateral(N, rng, step=BEHIND_STEP), g
    if family == "rotation":
        return gc.rotated_world(gc.pure_rotation(N, rng, rate=wc.ROTATION_RATE), g, gc.yaw(rng.uniform(0.0, 2.0 * np.pi)))
    return gc._poses(family, N, rng)


def make_wide_case(case):
    N, F, views, reverse = WIDE_FORM
    rng = np.random.default_rng([11, case.seed])
    poses, g = _wide_poses(case.family, N, rng)
    opts = {**gc._GATE, "views": views, "reverse": reverse, "gravity": g, **gc._OPTIONS[case.family]}
    return gc.make_geometry(poses, F, case.seed, **opts)


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(prob, oracle.update) of a case of GEOMETRY."""
    prob = make_wide_case(GEOMETRY[name])
    return prob, _update(prob)
