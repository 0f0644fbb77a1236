"""The failing batches of failing_batches.py mean what the GPU failure matrix (test_gpu_update_failures.py) assumes of them --
CPU only, NumPy against the oracle.  For every batch: every per-feature gate passes (reference MSCKF.py:561-568), and the
innovation covariance S = H P H^T + sigma^2 I is indefinite where the case says the update must fail and SPD where it must
not (a pivot of the sequential block Cholesky is non-positive exactly where a leading S is not SPD), with the remainder row
blocks on the side of the early launch's threshold the case intends."""
import numpy as np
import pytest

import failing_batches as fb
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
