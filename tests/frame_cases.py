"""Inputs shared by `test_gpu_tracks_frame.py`: the match list of its tests 2 and 3, and the way a store is grown from an
`UpdateProblem` (one clone at a time, `augment` + `tracks_observe`).  Not a conftest: imported by name.

The match list.  `synth.make_problem(31, 300, 31, variable_tracks=True, min_track=1)` plus a 32nd clone 1-2 mm from clone 15
(the homography branch runs against the views of that clone, the epipolar branch against all others), one keypoint per
track drawn uniformly from the image, and the two threshold pairs of `test_gpu_assoc.py`.  The new clone's rotation is
clone 15's turned by about 2e-3 rad: the reference's homography score compares a point with its own image under
`H = K R_12 K^-1` (`MSCKF.py:370-376`), about 180 px x the angle, more towards the image corners, so the second pair's 0.5 px
falls among the scores and a 31-view track passes or fails at its view 15 by where its keypoint lies.  Under the first
pair the signed epipolar score decides: a uniform keypoint is on the failing side of about half of a track's epipolar
lines, so the first failure is mostly early and rarely late.  `SEED` is a seed whose oracle output has every
property `assert_not_thin` lists (a failure at the last view of a 31-view track is the rare one); that is checked on the
CPU."""
import numpy as np

N, F, M = 31, 300, 31
SEED = 3042
PAIRS = ((1e-3, 150.0), (1e9, 0.5))      # (epipolar, homography) thresholds: test_gpu_assoc.py

J15 = np.zeros((6, 15))
J15[0:3, 0:3] = np.eye(3)
J15[3:6, 12:15] = np.eye(3)


def assoc_case(seed=SEED):
    """(prob, R_cur, t_cur, matched_uv (F, 2), score (F,))."""
    from msckf_amd import synth
    rng = np.random.default_rng(seed)
    prob = synth.make_problem(N, F, M, seed=seed, variable_tracks=True, min_track=1)
    R_cur = synth.so3_exp(2e-3 * rng.standard_normal(3)) @ prob.cam_R[N // 2]
    t_cur = prob.cam_t[N // 2] + 2e-3 * rng.standard_normal(3) / np.sqrt(3.0)
    muv = np.column_stack([rng.uniform(0, 640, F), rng.uniform(0, 480, F)])
    return prob, R_cur, t_cur, muv, rng.uniform(0.2, 1.0, F)


def assert_not_thin(prob, outs):
    """On the oracle's outputs alone (one (result, fail_view) per threshold pair): the inputs exercise the kernel."""
    nv = np.diff(prob.view_ptr)
    res = np.concatenate([o[0] for o in outs])
    fail = np.concatenate([o[1] for o in outs])
    nv = np.tile(nv, len(outs))
    assert int((res == 1).sum()) >= 5 and int((res == 2).sum()) >= 5
    assert ((res > 0) & (fail == 0)).any()                      # a failure at view 0
    assert ((res > 0) & (fail >= 16)).any()                     # one in the upper half of the group
    assert ((res > 0) & (nv == 31) & (fail == 30)).any()        # one at the last view of a 31-view track
    assert ((res == 0) & (nv == 31)).any()                      # a passing 31-view track


def grow_store(eng, prob, ids, score=None, P15=None):
    """The problem's tracks into the store, one clone at a time; `ids[j]` names track j.  Slot order is clone order."""
    vp, slot, uv = prob.view_ptr, np.asarray(prob.obs_slot), np.asarray(prob.obs_uv, dtype=np.float64)
    ids = np.asarray(ids)
    owner = np.repeat(np.arange(prob.F), np.diff(vp))
    eng.set_prior(np.eye(15) * 0.01 if P15 is None else P15, prob.gravity, prob.K, prob.sigma)
    for s in range(prob.N):
        eng.augment(J15, prob.cam_R[s], prob.cam_t[s])
        v = np.nonzero(slot == s)[0]
        eng.tracks_observe(ids[owner[v]], uv[v], np.ones(len(v)) if score is None else score[v])
