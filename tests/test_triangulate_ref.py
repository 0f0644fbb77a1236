"""The NumPy restatement of the refinement of triangulated points (`triangulate_ref`, the yardstick of
test_gpu_select_refine.py) on its own: it recovers known points, never raises the cost, leaves infeasible starts
alone and never touches the bits of the linear step.  No GPU.

Noise-free tolerance: 200 eps cond(A) relative, floor 1e-12, never looser than 1e-8 (A: the 3x3 normal matrix at the
point; the rule tests/test_gpu_select.py uses for the 3x3 solve of the linear step)."""
import numpy as np
import pytest

import triangulate_ref as tri

EPS = np.finfo(np.float64).eps


def _params(**kw):
    from msckf_amd import synth
    return synth.SelectParams(**dict(dict(use_parallax=False, min_frames_tracked=2), **kw))


def _noise_free(N, F, M, seed, variable=False):
    """A batch whose pixels are the exact projections of known world points through the batch's poses."""
    from msckf_amd import synth
    prob = synth.make_problem(N, F, M, seed=seed, pixel_noise=0.0, variable_tracks=variable, min_track=2)
    rng = np.random.default_rng(900 + seed)
    K = np.asarray(prob.K, dtype=np.float64)
    uv = np.array(prob.obs_uv, dtype=np.float64).reshape(-1, 2)
    points = np.zeros((F, 3))
    for j in range(F):
        a, b = int(prob.view_ptr[j]), int(prob.view_ptr[j + 1])
        slots = prob.obs_slot[a:b]
        while True:
            pc = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(4, 12)])
            pw = prob.cam_R[slots[0]] @ pc + prob.cam_t[slots[0]]
            q = np.einsum("mji,mj->mi", prob.cam_R[slots], pw[None, :] - prob.cam_t[slots])
            px = (q @ K.T)[:, :2] / q[:, 2:3]
            if (q[:, 2] > 0).all() and (px >= 0).all() and (px[:, 0] < synth.WIDTH).all() and (px[:, 1] < synth.HEIGHT).all():
                break
        points[j], uv[a:b] = pw, px
    prob.obs_uv = uv
    return prob, points


@pytest.mark.parametrize("N,F,M,seed,jitter,variable", [
    (8, 48, 6, 1, 0.005, False), (31, 24, 31, 5, 0.02, False), (6, 48, 2, 6, 0.01, False), (16, 80, 16, 7, 0.05, True)])
def test_noise_free_tracks_are_recovered(N, F, M, seed, jitter, variable):
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    prob, points = _noise_free(N, F, M, seed, variable)
    tracks = synth.make_tracks(prob, seed, lost_fraction=1.0, pose_jitter=jitter)      # the lines carry the jitter
    tracks.tracked_for = np.maximum(tracks.tracked_for, 2).astype(np.int32)
    lin = oracle.select_features(prob, tracks, _params())
    out = tri.refine_batch(prob, tracks, _params(), lin, 24)
    assert out["attempted"].sum() >= 0.8 * F
    moved = np.linalg.norm(lin["world"] - points, axis=1)
    assert np.median(moved[out["attempted"]]) > 1e-3                                    # the linear points are off ...
    for j in np.nonzero(out["attempted"])[0]:
        Ra, ta, Rs, ts, uv, w = tri.track_views(prob, tracks, j)
        C = Ra.T @ (points[j] - ta)
        x_true = np.array([C[0] / C[2], C[1] / C[2], 1.0 / C[2]])
        Kinv = np.linalg.inv(prob.K)
        A = tri.normal_equations(x_true, Ra, ta, Rs, ts, tri.normalised(uv, Kinv), w)[0]
        tol = min(max(200 * EPS * np.linalg.cond(A), 1e-12), 1e-8)
        assert out["kept"][j] and out["flags"][j] & tri.FLAG_REFINED
        err_w = np.linalg.norm(out["world"][j] - points[j]) / max(1.0, np.linalg.norm(points[j]))
        err_x = np.abs(out["x"][j] - x_true).max() / max(1.0, np.abs(x_true).max())
        assert err_w <= tol and err_x <= tol, (j, err_w, err_x, tol, int(out["trials"][j]))   # ... the refined ones are not


@pytest.mark.parametrize("N,F,M,seed,pk,tk,iters", [
    (8, 64, 6, 1, {}, dict(pose_jitter=0.005), 24),
    (6, 64, 2, 6, {}, dict(pose_jitter=0.01), 24),
    (16, 120, 16, 7, dict(variable_tracks=True, min_track=2), dict(pose_jitter=0.02, flip_fraction=0.2), 24),
    (16, 120, 16, 7, dict(variable_tracks=True, min_track=2), dict(pose_jitter=0.02, flip_fraction=0.2), 1),
    (10, 60, 8, 3, dict(outlier_fraction=0.2), dict(pose_jitter=0.05, flip_fraction=0.3), 3)])
def test_cost_never_increases_and_infeasible_starts_stay(N, F, M, seed, pk, tk, iters):
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(N, F, M, seed=seed, **pk)
    tracks = synth.make_tracks(prob, seed, lost_fraction=1.0, **tk)
    tracks.tracked_for = np.maximum(tracks.tracked_for, 2).astype(np.int32)
    lin = oracle.select_features(prob, tracks, _params())
    out = tri.refine_batch(prob, tracks, _params(), lin, iters)
    att, kept = out["attempted"], out["kept"]
    assert att.any() and (kept <= att).all()
    assert (out["cost1"][att] <= out["cost0"][att]).all() and (out["cost1"][kept] < out["cost0"][kept]).all()
    assert (out["trials"][att] >= 1).all() and out["trials"].max() <= iters
    for j in np.nonzero(kept)[0]:                                       # the reported costs are those of the points
        assert abs(tri.cost_at_world(prob, tracks, j, out["world"][j]) - out["cost1"][j]) <= 1e-9 * out["cost1"][j] + 1e-24
        assert abs(tri.cost_at_world(prob, tracks, j, lin["world"][j]) - out["cost0"][j]) <= 1e-9 * out["cost0"][j] + 1e-24
    stay = ~kept
    if "flip_fraction" in tk:
        assert (~att).any()                                             # lines crossing behind the cameras: no start
    for k in ("world", "idp_m", "idp_rho"):
        assert np.array_equal(out[k][stay], lin[k][stay], equal_nan=True), k
    assert not out["cost0"][~att].any() and not out["cost1"][~att].any() and not out["trials"][~att].any()
    assert not (out["flags"][stay] & tri.FLAG_REFINED).any()
    # a kept point is where its inverse-depth point says, in the reference's convention (unit m, rho = 1 / anchor depth)
    for j in np.nonzero(kept)[0]:
        a = int(prob.obs_slot[prob.view_ptr[j]])
        m = out["idp_m"][j]
        W = prob.cam_t[a] + m / (prob.cam_R[a].T @ m)[2] / out["idp_rho"][j]
        assert np.linalg.norm(W - out["world"][j]) <= 1e-8 * max(1.0, np.linalg.norm(W))


@pytest.mark.parametrize("sp,tk", [
    (dict(), dict(lost_fraction=0.5)),
    (dict(use_parallax=True, min_parallax_deg=3.0, min_frames_tracked=5), dict(lost_fraction=0.4, flip_fraction=0.2)),
    (dict(width=400, height=300), dict(lost_fraction=1.0, pose_jitter=0.05))])
def test_bits_of_the_linear_step_stay(sp, tk):
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(12, 150, 9, seed=21, variable_tracks=True, min_track=1)
    tracks = synth.make_tracks(prob, 21, **tk)
    params = _params(**sp)
    lin = oracle.select_features(prob, tracks, params)
    for iters in (1, 24):
        out = tri.refine_batch(prob, tracks, params, lin, iters)
        assert np.array_equal(out["flags"] & 7, lin["flags"])
        assert np.array_equal((out["flags"] & 8) > 0, out["kept"]) and out["kept"].any()
        assert not (out["kept"] & ((lin["flags"] & 5) != 5)).any()      # a refined track was valid and refreshed
    assert (lin["flags"] & 7 != 5).any()                                # ... and the batch holds tracks that were not
    off = tri.refine_batch(prob, tracks, params, lin, 0)
    assert not off["kept"].any() and np.array_equal(off["flags"], lin["flags"])


def test_long_double_agrees_with_fp64():
    """The two precisions of the restatement tell the same story: same kept set, points within 1e-6 relative."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(8, 64, 6, seed=1)
    tracks = synth.make_tracks(prob, 1, lost_fraction=1.0, pose_jitter=0.005)
    tracks.tracked_for = np.maximum(tracks.tracked_for, 2).astype(np.int32)
    lin = oracle.select_features(prob, tracks, _params())
    a = tri.refine_batch(prob, tracks, _params(), lin, 24)
    b = tri.refine_batch(prob, tracks, _params(), lin, 24, np.longdouble)
    assert np.array_equal(a["kept"], b["kept"]) and a["kept"].all()
    assert b["x"].dtype == np.longdouble and np.finfo(np.longdouble).eps < EPS
    assert tri.rel_spread(a["world"], b["world_hi"]).max() < 1e-6 and tri.rel_spread(a["x"], b["x"]).max() < 1e-6
