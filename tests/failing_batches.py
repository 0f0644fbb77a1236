"""Batches whose per-feature gates all pass but whose joint innovation covariance is indefinite: K6-K7's sequential
16-row block update meets a pivot that is not a positive normal number and must report MSCKF_ERR_NOT_SPD (a numerical
status, not a device fault).  Shared by the CPU precondition test (test_failing_batches.py) and the GPU failure matrix
(test_gpu_update_failures.py).  Not a conftest: imported by name.

The twin recipe: a problem of n clones and tracks of 16 - n views (more than 15 slots: every one is split into two view
groups -- narrow blocks + three remainder rows; a track of up to 15 slots rides the band plan whole), its
poses tiled twice into a window of 2n clones, its tracks taken once as they are and once shifted by n slots.  P = p I with every clone component k of clone i coupled to the same component of its twin
i + n by +-c, the sign alternating with k.  No track sees both twins, so every gate matrix is SPD (each half of P is p I);
the stacked rows see both, and with c > p the joint S is indefinite.

The hole variant: tracks of n views of which views 0 - 6 and the last are kept, coupling on the last clone (and its twin)
alone.  That view is a view group of its own: two carry rows and no narrow block, so only the remainder rows see the
coupled clones -- the narrow rows (the band root's) are SPD, the update on the remainder rows behind them is not."""
import numpy as np

from msckf_amd import synth
from oracle import msckf_oracle as oracle

SPLIT_SLOTS = 10          # SPLIT_GSLOTS of csrc/k_feature.h: the widest view group of a split track
SPLIT_SPAN = 15           # a track over more slots than this is split (up to it: 90-column band tiles)
T2_EARLY_MIN = 20         # t2_early_min() of msckf_abi.hip: remainder row blocks from which they get a launch of their own

# name: (clones of one half, tracks of one half, seed, p, c[, hole]).  What each is for is pinned by test_failing_batches.py.
TWINS = {
    "early": (17, 80, 5, 1e-2, 5e-2),        # N = 34, 160 tracks, 60 remainder row blocks: the early launch (k_gain_dense) fails
    "root": (17, 80, 5, 5e-4, 2e-3),         # the same tracks, a weaker prior: the remainder rows are SPD, the root's launch fails
    "inroot": (17, 20, 5, 1e-2, 5e-2),       # 40 tracks, 15 blocks: remainder rows inside the root's launch, and they fail there
    "wide": (20, 80, 7, 1e-2, 5e-2),         # N = 40 (16 strips): the early launch on k_gain_stream, not k_gain_dense
    "hole": (17, 80, 5, 1e-2, 5e-2, True),   # narrow rows SPD, remainder rows not: the update on the remainder rows fails
}


def twin_problem(n, F, seed, p, c, hole=False):
    if hole:
        b = synth.make_problem(n, F, n, seed=seed)
        keep = np.array(list(range(7)) + [n - 1])
        idx = np.concatenate([b.view_ptr[j] + keep for j in range(F)])
        a = synth.UpdateProblem(**{**b.__dict__, "view_ptr": (np.arange(F + 1) * len(keep)).astype(np.int32),
                                   "obs_uv": b.obs_uv[idx], "obs_slot": b.obs_slot[idx]})
    else:
        a = synth.make_problem(n, F, n, seed=seed, variable_tracks=True, min_track=16)
    two = lambda x: np.concatenate([x, x])
    vp = np.concatenate([a.view_ptr, a.view_ptr[-1] + a.view_ptr[1:]]).astype(np.int32)
    N = 2 * n
    d = 15 + 6 * N
    P = p * np.eye(d)
    for i in ([n - 1] if hole else range(n)):
        for k in range(6):
            u, v = 15 + 6 * i + k, 15 + 6 * (i + n) + k
            P[u, v] = P[v, u] = c if k % 2 == 0 else -c
    return synth.UpdateProblem(
        P=P, cam_R=two(a.cam_R), cam_t=two(a.cam_t), cam_R0=two(a.cam_R0), cam_t0=two(a.cam_t0), gravity=a.gravity,
        K=a.K, sigma=a.sigma, view_ptr=vp, obs_uv=two(a.obs_uv),
        obs_slot=np.concatenate([a.obs_slot, a.obs_slot + n]).astype(np.int32),
        idp_base=two(a.idp_base), idp_m=two(a.idp_m), idp_rho=two(a.idp_rho),
        meta={"N": N, "F": 2 * F, "twin": (n, F, seed, p, c, hole)})


def twin(name):
    return twin_problem(*TWINS[name])


def spd_p_problem(N=30, F=300, M=10, seed=64):
    """A short-track batch (nothing split) whose 180 x 180 innovation covariance is indefinite: the prior's 10-clone
    diagonal blocks stay SPD, clone 0 and clone 29 are coupled by +-50 (no track sees both)."""
    prob = synth.make_problem(N, F, M, seed=seed)
    P = 1e-3 * np.eye(prob.d)
    P[15, 15 + 6 * (N - 1)] = P[15 + 6 * (N - 1), 15] = 50.0
    P[18, 18 + 6 * (N - 1)] = P[18 + 6 * (N - 1), 18] = -50.0
    prob.P = P
    return prob


# run_select in front of the update: every track lost and tracked long enough, no parallax test -> every track is valid and
# gets its inverse-depth point refreshed from its lines (no pose jitter: the lines go through the clone positions)
SELECT = synth.SelectParams(min_frames_tracked=2, use_parallax=False)


def select_tracks(prob):
    return synth.make_tracks(prob, seed=1, lost_fraction=1.0, pose_jitter=0.0)


def selected(prob, tracks):
    """(the valid tracks, the batch the update behind run_select sees: those tracks with their refreshed points)."""
    sel = oracle.select_features(prob, tracks, SELECT)
    valid = np.nonzero(sel["flags"] & 1)[0]
    sub = synth.UpdateProblem(**{**prob.__dict__, "idp_m": sel["idp_m"], "idp_rho": sel["idp_rho"]}).take(valid)
    return valid, sub


def view_groups(slots):
    """The library's view groups of one track (msckf_set_features): ceil(span / 10) stretches, empty ones skipped."""
    lo, hi = int(slots.min()), int(slots.max())
    span = hi - lo + 1
    ng0 = (span + SPLIT_SLOTS - 1) // SPLIT_SLOTS
    out, v = [], 0
    for g0 in range(ng0):
        bnd = lo + ((g0 + 1) * span) // ng0
        v0 = v
        while v < len(slots) and slots[v] < bnd:
            v += 1
        if v > v0:
            out.append((v0, v))
    return out


def remainder_blocks(prob):
    """Row blocks of the remainder rows' capacity (3 per view group of every split track), as the early launch counts them."""
    cap = 0
    for j in range(prob.F):
        slots = np.asarray(prob.obs_slot[prob.view_ptr[j]:prob.view_ptr[j + 1]])
        if slots.max() - slots.min() + 1 > SPLIT_SPAN:
            cap += 3 * len(view_groups(slots))
    return (cap + 15) // 16
