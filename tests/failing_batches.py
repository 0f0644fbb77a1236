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
coupled clones -- the narrow rows (the band root's) are SPD, the update on the remainder rows behind them is not.

The other way round -- gate matrices that are NOT SPD under a joint S that is -- is gate_not_spd_problem (GATE_CASES): the
rows and columns of P of one clone slot a are zero but for its 6 x 6 block, which is -c I.  A track without a view in
clone a has H_o zero on those columns: its S_j is what it was, and the joint S of any set of such tracks is SPD.  A track
that sees clone a gets S_j = (SPD part) - c A A^T + sigma^2 I with A its rows' clone-a block: indefinite by a wide margin at
c = 1 (test_failing_batches.py pins lambda_min <= -10 sigma^2), and by Sylvester's law of inertia so in every basis of the
null space, so an elimination without pivoting meets a non-positive pivot whatever basis k_feature uses.  Such a track
ends in gate byte 2: dropped before the chi-square test, counted in not_spd and not in n_rejected, and the update is that
of the batch without it (the oracle on prob.take(good); the oracle on the whole batch inverts the indefinite S_j as NumPy
does, MSCKF.py:561-568, and is no reference here)."""
import numpy as np

from msckf_amd import synth
from oracle import msckf_oracle as oracle

SPLIT_SLOTS = 10          # SPLIT_GSLOTS of csrc/batch_order.h: the widest view group of a split track
SPLIT_SPAN = 15           # TILE_SPAN of csrc/batch_order.h: a track over more slots than this is split (up to it: 90-column band tiles)
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
    """The library's view groups of one track (for_each_group of csrc/batch_order.h): ceil(span / 10) stretches, empty ones skipped."""
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


def remainder_blocks(prob, split=None):
    """Row blocks of the remainder rows' capacity (3 per view group of every split track), as the early launch counts them.
    split: the mask of the split tracks (long_tracks); default: every track over more than 15 slots."""
    cap = 0
    for j in range(prob.F):
        slots = np.asarray(prob.obs_slot[prob.view_ptr[j]:prob.view_ptr[j + 1]])
        if (slots.max() - slots.min() + 1 > SPLIT_SPAN) if split is None else split[j]:
            cap += 3 * len(view_groups(slots))
    return (cap + 15) // 16


# ---- gate matrices that are not SPD (gate byte 2) ----------------------------------------------------------------------
WIDE_SPAN = 10            # WIDE_SPAN of csrc/batch_order.h: a track over more slots is long (split when its views come in slot order)
REM_DIRECT_MID = 2048     # MID_DIRECT_ROWS of csrc/batch_order.h: remainder rows (6 per 11 - 15-slot track) up to which a batch without a longer track is still split

# name: (N, F, M, seed, clone a, make_problem options, every track's views reversed,
#        (shortest, longest track in views) -- the k_feature instance the batch's unsplit tracks reach:
#        <= 10 views <24>, <= 15 <32>, more <64> --, long tracks among the bad / the good (None: none at all),
#        the good sub-batch has gate-rejected tracks).  Pinned by test_failing_batches.py.
_RAGGED = {"variable_tracks": True, "min_track": 2}
_OUTLIERS = {"outlier_fraction": 0.15, "outlier_px": 300.0}
GATE_CASES = {
    "k24": (12, 60, 6, 7, 5, _RAGGED, False, (2, 6), None, False),
    "k32": (16, 40, 15, 7, 0, {"variable_tracks": True, "min_track": 11, **_OUTLIERS}, False, (11, 15), None, True),
    "k64": (20, 40, 20, 7, 19, {"variable_tracks": True, "min_track": 16, **_OUTLIERS}, True, (16, 20), None, True),
    "split": (31, 120, 31, 7, 17, _RAGGED, False, (2, 30), True, False),
    "mixed": (30, 200, 10, 7, 29, {**_RAGGED, **_OUTLIERS}, False, (2, 10), None, True),
    "all_bad": (12, 40, 12, 7, 6, {}, False, (12, 12), None, False),
    # the one case past 31 clones, for an engine with plan="tree": leaves wider than the 186 columns k_fold keeps in LDS go to
    # k_fold_g, which no window of up to 31 clones reaches
    "tree_wide": (34, 40, 31, 7, 33, {"variable_tracks": True, "min_track": 25, **_OUTLIERS}, False, (25, 31), None, True),
}
FOLD_LDS_COLUMNS = 186    # FOLD_RLDS_MAX_W of k_fold.h


def reverse_views(prob):
    """Every track's views in descending slot order: a long track then keeps ONE block (the groups of a split are view ranges)."""
    uv, sl = prob.obs_uv.copy(), prob.obs_slot.copy()
    for j in range(prob.F):
        a, b = int(prob.view_ptr[j]), int(prob.view_ptr[j + 1])
        uv[a:b] = uv[a:b][::-1]
        sl[a:b] = sl[a:b][::-1]
    return synth.UpdateProblem(**{**prob.__dict__, "obs_uv": uv, "obs_slot": sl})


def gate_not_spd_problem(N, F, M, seed, a, c=1.0, reverse=False, **make_problem_options):
    """(prob, bad_mask): a synth.make_problem batch whose prior has clone a cut off and its block set to -c I; bad_mask marks
    the tracks with a view in clone a."""
    prob = synth.make_problem(N, F, M, seed=seed, **make_problem_options)
    P = prob.P.copy()
    i = 15 + 6 * a
    P[i:i + 6, :] = 0.0
    P[:, i:i + 6] = 0.0
    P[i:i + 6, i:i + 6] = -c * np.eye(6)
    prob.P = P
    if reverse:
        prob = reverse_views(prob)
    return prob, sees_clone(prob, a)


def gate_lambda(prob):
    """lambda_min(S_j) / sigma^2 of every track's gate matrix (oracle basis; its sign pattern is that of every basis)."""
    s2 = prob.sigma ** 2
    lam = np.zeros(prob.F)
    for j in range(prob.F):
        r, Hx, Hf = oracle.feature_blocks(prob, j)
        _, Ho = oracle.project_on_nullspace(Hf, r, Hx)
        lam[j] = np.linalg.eigvalsh(Ho @ prob.P @ Ho.T + s2 * np.eye(Ho.shape[0])).min() / s2
    return lam


def sees_clone(prob, a):
    return np.array([a in prob.obs_slot[prob.view_ptr[j]:prob.view_ptr[j + 1]] for j in range(prob.F)], dtype=bool)


def gate_case(name):
    N, F, M, seed, a, kw, rev = GATE_CASES[name][:7]
    return gate_not_spd_problem(N, F, M, seed, a, reverse=rev, **kw)


def long_tracks(prob):
    """The tracks msckf_set_features splits (default plan, one context): more than 10 slots, views in slot order; none when no
    track spans more than 15 slots and most span 11 - 15 (or their remainder rows would be too many): 90-column tiles instead."""
    out = np.zeros(prob.F, dtype=bool)
    n_mid = n_long = 0
    for j in range(prob.F):
        sl = np.asarray(prob.obs_slot[prob.view_ptr[j]:prob.view_ptr[j + 1]])
        span = int(sl.max() - sl.min() + 1)
        n_long += span > SPLIT_SPAN
        n_mid += WIDE_SPAN < span <= SPLIT_SPAN
        out[j] = span > WIDE_SPAN and bool(np.all(np.diff(sl) > 0))
    if prob.N <= WIDE_SPAN or (out.any() and n_long == 0 and (2 * n_mid > prob.F or 6 * n_mid > REM_DIRECT_MID)):
        out[:] = False
    return out


# run_select in front of the "mixed" gate case: 40 % of the tracks are not lost, hence not valid (gate byte 3)
GATE_SELECT = synth.SelectParams(min_frames_tracked=2, use_parallax=False)


def gate_select_tracks(prob):
    return synth.make_tracks(prob, seed=7, lost_fraction=0.6)


def gate_selected(prob, tracks, bad, params=GATE_SELECT):
    """The oracle chain of test_select_against_oracle restricted to the valid tracks that are good:
    (selection, valid mask, indices of the valid good tracks, oracle.update on them with their refreshed points)."""
    sel = oracle.select_features(prob, tracks, params)
    valid = (sel["flags"] & 1) > 0
    idx = np.nonzero(valid & ~bad)[0]
    chained = prob.take(idx)
    chained.idp_m, chained.idp_rho = sel["idp_m"][idx], sel["idp_rho"][idx]
    return sel, valid, idx, oracle.update(chained, dense_noise=False)


def without_clone(prob, a):
    """The batch after remove_clones([a]) (P and poses aside): views in clone a gone, later slots moved down.
    Returns (view_ptr, obs_uv, obs_slot, indices of the tracks that have views left)."""
    keep_v = np.asarray(prob.obs_slot) != a
    n_left = np.add.reduceat(keep_v.astype(np.int64), prob.view_ptr[:-1])
    left = np.nonzero(n_left > 0)[0]
    sl = np.asarray(prob.obs_slot)[keep_v]
    vp = np.concatenate([[0], np.cumsum(n_left[left])]).astype(np.int32)
    return vp, prob.obs_uv[keep_v], (sl - (sl > a)).astype(np.int32), left
