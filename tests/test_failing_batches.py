"""The failing batches of failing_batches.py mean what the GPU failure matrix (test_gpu_update_failures.py) assumes of them --
CPU only, NumPy against the oracle.  For every batch: every per-feature gate passes (reference MSCKF.py:561-568), and the
innovation covariance S = H P H^T + sigma^2 I is indefinite where the case says the update must fail and SPD where it must
not (a pivot of the sequential block Cholesky is non-positive exactly where a leading S is not SPD), with the remainder row
blocks on the side of the early launch's threshold the case intends.

The gate cases (failing_batches.GATE_CASES) are the other way round: the tracks that see the cut-off clone have an indefinite
gate matrix S_j by a wide margin, every other track an SPD one, no track lies in between, and the update of the good tracks
alone is an ordinary one -- what test_gpu_gate_not_spd.py assumes of them."""
import numpy as np
import pytest

import failing_batches as fb
from msckf_amd import synth
from oracle import msckf_oracle as oracle
from test_split_math import split_track


def _min_eig(H, P, s2):
    if H.shape[0] > P.shape[0]:
        H = np.linalg.qr(H, mode="r")             # (same negative eigenvalues: H = Q R)
    return float(np.linalg.eigvalsh(H @ P @ H.T + s2 * np.eye(H.shape[0])).min())


def _rows(prob):
    """(gates passed, the projected rows of every track, its narrow rows, its remainder rows) -- the two-level basis of
    k_feature<64, true> for the split tracks (test_split_math.py)."""
    n_pass, Hs, Hn, Hr = 0, [], [], []
    for j in range(prob.F):
        r, Hx, Hf = oracle.feature_blocks(prob, j)
        ro, Ho = oracle.project_on_nullspace(Hf, r, Hx)
        n_pass += int(oracle.gate(ro, Ho, prob.P, prob.sigma)[0])
        Hs.append(Ho)
        narrow, rem = split_track(prob, j)
        Hn += [h for h, _ in narrow]
        Hr.append(rem[0])
    return n_pass, np.vstack(Hs), np.vstack(Hn), np.vstack(Hr)


# name: (early launch (>= 20 remainder blocks), S over the remainder rows SPD, S over the narrow rows SPD)
CASES = {
    "early": (True, False, None),      # the early launch itself meets the bad pivot
    "root": (True, True, None),        # the early launch succeeds; the update on the root, behind it, fails
    "inroot": (False, False, None),    # the remainder rows inside the root's launch, and they fail
    "wide": (True, False, None),       # N = 40
    "hole": (True, False, True),       # narrow rows SPD: with the remainder tree, the second update (chain) fails
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("select", [False, True])
def test_twin_batches_pass_every_gate_and_fail_jointly(name, select):
    prob = fb.twin(name)
    if select:                                  # the batch the update behind run_select sees
        valid, prob = fb.selected(prob, fb.select_tracks(prob))
        assert len(valid) == fb.twin(name).F
    early, rem_spd, narrow_spd = CASES[name]
    n_pass, Hs, Hn, Hr = _rows(prob)
    s2 = prob.sigma ** 2
    assert n_pass == prob.F
    assert (fb.remainder_blocks(prob) >= fb.T2_EARLY_MIN) == early
    assert _min_eig(Hs, prob.P, s2) < -1e-3                          # the whole stack: indefinite
    e_rem = _min_eig(Hr, prob.P, s2)
    assert (e_rem > 1e-3) if rem_spd else (e_rem < -1e-3), e_rem
    if narrow_spd is not None:
        assert _min_eig(Hn, prob.P, s2) > 1e-3


@pytest.mark.parametrize("select", [False, True])
def test_short_track_batch_passes_every_gate_and_fails_jointly(select):
    prob = fb.spd_p_problem()
    if select:
        valid, prob = fb.selected(prob, fb.select_tracks(prob))
        assert len(valid) == fb.spd_p_problem().F
    n_pass, Hs = 0, []
    for j in range(prob.F):
        r, Hx, Hf = oracle.feature_blocks(prob, j)
        ro, Ho = oracle.project_on_nullspace(Hf, r, Hx)
        n_pass += int(oracle.gate(ro, Ho, prob.P, prob.sigma)[0])
        Hs.append(Ho)
    assert n_pass == prob.F
    assert fb.remainder_blocks(prob) == 0
    assert _min_eig(np.vstack(Hs), prob.P, prob.sigma ** 2) < -1e-3


# ---- gate matrices that are not SPD: what test_gpu_gate_not_spd.py assumes of GATE_CASES -------------------------------
BAD_MAX = -10.0      # lambda_min(S_j) / sigma^2 of every track that sees the cut-off clone: at most this
GOOD_MIN = 0.5       # ... of every other track: at least this (sigma^2 I alone gives 1)

# long tracks / remainder row blocks each case must give the library to plan (None: no long track)
# ("tree": the case is for plan="tree", which splits nothing)
GATE_SPLIT = {"k24": None, "k32": None, "k64": None, "mixed": None, "all_bad": None, "split": (73, 35), "tree_wide": "tree"}


@pytest.mark.parametrize("name", sorted(fb.GATE_CASES))
def test_gate_cases_classify_every_track(name):
    N, F, M, seed, a, kw, rev, lens, long_sides, rejects = fb.GATE_CASES[name]
    prob, bad = fb.gate_case(name)
    assert prob.N == N and prob.F == F <= 200 and (N <= 31 or name == "tree_wide") and bad.shape == (F,)
    lam = fb.gate_lambda(prob)
    good = ~bad
    print("%s: %d bad tracks, lambda_min / sigma^2 <= %.2f; %d good ones, >= %.3f"
          % (name, bad.sum(), lam[bad].max(), good.sum(), lam[good].min() if good.any() else np.nan))
    assert bad.any() and (lam[bad] <= BAD_MAX).all()
    assert (lam[good] >= GOOD_MIN).all()
    assert not ((lam > BAD_MAX) & (lam < GOOD_MIN)).any()                    # no track is unclassified
    # the prior without clone a is untouched, so the good tracks' S_j are those of the original prior
    orig = synth.make_problem(N, F, M, seed=seed, **kw)
    i = 15 + 6 * a
    keep = np.r_[0:i, i + 6:prob.d]
    assert np.array_equal(prob.P[np.ix_(keep, keep)], orig.P[np.ix_(keep, keep)])
    assert np.array_equal(prob.P[i:i + 6, i:i + 6], -np.eye(6)) and not prob.P[i:i + 6, keep].any()
    # the kernel form: the track-length class, the long tracks and their remainder rows
    n_views = np.diff(prob.view_ptr)
    assert (int(n_views.min()), int(n_views.max())) == lens
    long = fb.long_tracks(prob)
    assert bool(long_sides) == isinstance(GATE_SPLIT[name], tuple)
    if GATE_SPLIT[name] == "tree":
        # every track of the batch fits no window of 31 clones: whatever leaves the tree plan forms, one is wider than k_fold's LDS
        first = np.minimum.reduceat(prob.obs_slot, prob.view_ptr[:-1])
        last = np.maximum.reduceat(prob.obs_slot, prob.view_ptr[:-1])
        assert 6 * (int(last.max()) - int(first.min()) + 1) > fb.FOLD_LDS_COLUMNS
    elif GATE_SPLIT[name] is None:
        assert not long.any()
    else:
        assert (int(long.sum()), fb.remainder_blocks(prob, long)) == GATE_SPLIT[name]
        assert (long & bad).any() and (long & good).any() and (~long & bad).any() and (~long & good).any()
        assert long.sum() <= 512                                             # four wavefronts per track by default
        assert fb.remainder_blocks(prob, long) >= fb.T2_EARLY_MIN
    if name == "all_bad":
        assert bad.all()
        return
    ref = oracle.update(prob.take(np.nonzero(good)[0]), dense_noise=False)
    n_acc = int(ref["accepted"].sum())
    print("    good sub-batch: status %d, %d of %d accepted" % (ref["status"], n_acc, good.sum()))
    assert ref["status"] == 0 and n_acc > 0
    if rejects:
        assert n_acc < good.sum()
    # the joint S of the good tracks that pass: SPD (what K6-K7 factorises)
    assert np.linalg.eigvalsh(ref["T_H"] @ prob.P @ ref["T_H"].T + prob.sigma ** 2 * np.eye(ref["T_H"].shape[0])).min() > 0.5 * prob.sigma ** 2


def test_gate_case_with_a_weak_block_would_not_classify():
    """Why c stays at 1: with c = 0.01 some tracks that see the clone keep an SPD gate matrix or land close to zero."""
    N, F, M, seed, a, kw = fb.GATE_CASES["k24"][:6]
    prob, bad = fb.gate_not_spd_problem(N, F, M, seed, a, c=0.01, **kw)
    lam = fb.gate_lambda(prob)
    assert (lam[bad] > BAD_MAX).any()


def test_mixed_case_behind_run_select_holds_all_four_gate_bytes():
    """The batch k_feature sees behind run_select (refreshed points): not valid (3), valid and bad (2), valid and good on
    both sides of the chi-square test (0, 1) -- and the refreshed points leave every valid track classified."""
    prob, bad = fb.gate_case("mixed")
    sel, valid, idx, ref = fb.gate_selected(prob, fb.gate_select_tracks(prob), bad)
    assert (~valid).any() and (valid & bad).any() and (~valid & bad).any()
    assert ref["status"] == 0 and 0 < int(ref["accepted"].sum()) < len(idx)
    full = synth.UpdateProblem(**{**prob.__dict__, "idp_m": sel["idp_m"], "idp_rho": sel["idp_rho"]}).take(np.nonzero(valid)[0])
    lam, vb = fb.gate_lambda(full), bad[valid]
    print("behind run_select: bad <= %.2f, good >= %.3f" % (lam[vb].max(), lam[~vb].min()))
    assert (lam[vb] <= BAD_MAX).all() and (lam[~vb] >= GOOD_MIN).all()


def test_split_case_stays_classified_over_commits_and_a_removed_clone():
    """Commit and go on: the oracle's P+ of the good tracks keeps the -I block of clone a (their rows are zero there), so the
    same batch on the committed prior classifies the same way twice; with clone a removed every gate matrix is SPD."""
    prob, bad = fb.gate_case("split")
    a = fb.GATE_CASES["split"][4]
    good = np.nonzero(~bad)[0]
    i = 15 + 6 * a
    P = prob.P
    for step in range(2):
        ref = oracle.update(synth.UpdateProblem(**{**prob.__dict__, "P": P}).take(good), dense_noise=False)
        assert ref["status"] == 0
        P = ref["P_new"]
        assert np.array_equal(P[i:i + 6, i:i + 6], -np.eye(6)) and not np.delete(P[i:i + 6], np.s_[i:i + 6], axis=1).any()
        lam = fb.gate_lambda(synth.UpdateProblem(**{**prob.__dict__, "P": P}))
        print("after commit %d: bad <= %.2f, good >= %.3f" % (step + 1, lam[bad].max(), lam[~bad].min()))
        assert (lam[bad] <= BAD_MAX).all() and (lam[~bad] >= GOOD_MIN).all()
    vp, uv, sl, left = fb.without_clone(prob, a)
    assert len(left) == prob.F                                               # (every track has at least two views)
    keep = np.delete(np.arange(prob.N), a)
    q = synth.UpdateProblem(**{**prob.__dict__, "P": oracle.remove_clones_covariance(P, [a]), "cam_R": prob.cam_R[keep],
                               "cam_t": prob.cam_t[keep], "cam_R0": prob.cam_R0[keep], "cam_t0": prob.cam_t0[keep],
                               "view_ptr": vp, "obs_uv": uv, "obs_slot": sl})
    assert (fb.gate_lambda(q) >= GOOD_MIN).all()
    assert np.linalg.eigvalsh(q.P).min() > 0
