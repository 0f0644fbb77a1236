"""The reference's 30-clone filter run (`golden/window30/seq_window30.npz`, loader `window30.py`) on the engine.

(a) Resident: the covariance is uploaded once (`set_prior`) and never again -- propagate, augment, select + update +
commit on the frame's batch, prune, remove clones -- and must stay on the reference's covariance through every op.
(b) Drop-in: the same frames through `UpdateEngine.process_features(filt)` and `prune_poorest_camera_states(filt)` on
reference-shaped objects that alias their lines' and inverse-depth points' bases to the clones' position arrays as the
reference does (`MSCKF.py:410, :430-431`), so every injection moves them (`inject.py`'s in-place `+=`).

Tolerances: flags, masks, status and counters exact; refreshed points as in test_gpu_select.check_selection; dx 1e-8
relative; probes P @ V and checkpoints 1e-8 relative with P exactly symmetric; poses after injection 1e-9."""
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import rel_err
import window30
from window30 import AUGMENT, IMU, PROCESS, PRUNE, REMOVE
from test_gpu_select import check_selection

pytestmark = pytest.mark.gpu

TOL = 1e-8
POSE_TOL = 1e-9


@pytest.fixture(scope="module")
def run():
    return window30.Run()


@pytest.fixture(scope="module")
def eng():
    from msckf_amd.api import UpdateEngine
    e = UpdateEngine(max_clones=31, max_features=4096, max_track=31)
    yield e
    e.close()


def _imu_step(run, eng, idx):
    from msckf_amd import propagation
    z, s = run.z, run.imu(idx)
    Phi, Q = propagation.imu_transition(s["R"], s["t"], s["v"], s["R0"], s["t0"], s["v0"], s["gyro"], s["acc"],
                                        float(s["dt"]), z["gravity"], z["Qc"], s["w_planet"])
    eng.propagate(Phi, Q)


def _augment(run, eng, idx):
    from msckf_amd import propagation
    z, a = run.z, run.aug(idx)
    J, cR, ct = propagation.augmentation(a["imu_R"], a["imu_t"], (z["T_W_I_R"], z["T_W_I_t"]), (z["T_W_C_R"], z["T_W_C_t"]))
    np.testing.assert_allclose(cR, a["cam_R"], atol=1e-13)
    np.testing.assert_allclose(ct, a["cam_t"], atol=1e-13)
    eng.augment(J, cR, ct)
    return a


def _check_probe(run, o, P, worst):
    if o in run.probes:
        e = rel_err(P @ run.V[:P.shape[0]], run.probes[o])
        worst["probe"] = max(worst["probe"], e)
        assert e < TOL, (o, e)
    if o in run.checkpoints:
        e = rel_err(P, run.checkpoints[o])
        worst["probe"] = max(worst["probe"], e)
        assert e < TOL, (o, e)


def test_resident_window30_run_tracks_the_reference(run, eng):
    from oracle import msckf_oracle as oracle
    z = run.z
    params = run.select_params()
    eng.set_prior(z["P0"], z["gravity"], z["K"], run.sigma)
    keys, cam_R, cam_t = [], np.zeros((0, 3, 3)), np.zeros((0, 3))
    worst = dict(dx=0.0, probe=0.0)
    split_updates = updates = 0
    for o, (kind, idx) in enumerate(run.ops):
        if kind == IMU:
            _imu_step(run, eng, idx)
        elif kind == AUGMENT:
            a = _augment(run, eng, idx)
            keys.append(int(a["key"]))
            cam_R, cam_t = np.concatenate([cam_R, a["cam_R"][None]]), np.concatenate([cam_t, a["cam_t"][None]])
        elif kind in (PROCESS, PRUNE):
            c = run.call(idx)
            assert c["keys"].tolist() == keys and eng.n_clones == len(keys)
            if kind == PRUNE:
                poorest = window30.poorest_two(c["counts"])
                assert sorted(keys.index(k) for k in poorest) == c["rm"].tolist()
            prob = run.problem(c, np.zeros((15 + 6 * len(keys),) * 2), cam_R, cam_t)
            tracks = run.tracks(c)
            eng.set_features(prob)                           # only the batch travels; P and poses are resident
            eng.set_tracks(tracks)
            eng.run_select(params, prob.K)
            sel = eng.selection()
            cond = oracle.select_features(prob, tracks, params)["cond"]
            check_selection(sel, c["flags"], c["sel_m"], c["sel_rho"], c["world"], cond)
            n_valid = int(sel.valid.sum())
            if 0 < n_valid < 0.15 * prob.F:
                eng.replan()                                 # as process_features does (api.py)
            if n_valid:
                eng.run()
                res = eng.result()
                assert res.status == c["status"] and res.n_rejected == c["n_rejected"]
                assert np.array_equal(res.accepted, c["accepted"])
                if res.status == 0:
                    updates += 1
                    e = rel_err(res.dx, c["dx"])
                    worst["dx"] = max(worst["dx"], e)
                    assert e < TOL, (o, e)
                    split_updates += int(eng.debug_split()["long_tracks"] > 0)
                assert eng.commit_covariance() == res.status
            else:
                assert c["status"] == 1
            if kind == PRUNE:
                eng.remove_clones(c["rm"])
                keys = [k for s, k in enumerate(keys) if s not in c["rm"]]
            cam_R, cam_t = c["post_R"].copy(), c["post_t"].copy()
            if c["status"] == 0:
                eng.set_poses(cam_R, cam_t)                  # poses after the host's injection
        elif kind == REMOVE:
            c = run.call(idx)
            eng.remove_clones(c["rm"])
            keep = [s for s in range(len(keys)) if s not in c["rm"]]
            keys, cam_R, cam_t = [keys[s] for s in keep], cam_R[keep], cam_t[keep]
        assert eng.n_clones == len(keys)
        if o in run.probes or o in run.checkpoints:
            P = eng.covariance()
            assert np.array_equal(P, P.T)
            _check_probe(run, o, P, worst)
    assert split_updates >= 10, split_updates
    print(f"resident window30: {updates} updates, {split_updates} with split long tracks; "
          f"worst dx {worst['dx']:.2e}, probes {worst['probe']:.2e}")


# ---- (b) the drop-in calls on reference-shaped objects -------------------------------------------------------------
def _remove_cameras(filt, drop):
    """The reference's `remove_cameras` (`MSCKF.py:751-779`) on the test's objects."""
    cams = filt.state.cameras
    for k in drop:
        i = list(cams.keys()).index(k)
        P = np.delete(filt.state.covariance, slice(15 + 6 * i, 21 + 6 * i), axis=0)
        filt.state.covariance = np.delete(P, slice(15 + 6 * i, 21 + 6 * i), axis=1)
        del cams[k]
    gone = []
    for fid, ft in filt.features.items():
        for k in drop:
            if k in ft.camera_indices:
                v = ft.camera_indices.index(k)
                for name in ("keypoints", "descriptors", "scores", "camera_indices", "lines"):
                    del getattr(ft, name)[v]
        if not ft.camera_indices:
            gone.append(fid)
    for fid in gone:
        del filt.features[fid]


def _make_filter(run):
    z = run.z
    params = run.select_params()
    imu = SimpleNamespace(W_gravity=z["gravity"].copy(), T_W_Ii=SimpleNamespace(R=np.eye(3), t=np.zeros(3)),
                          v_W_Ii=np.zeros(3), gyroscope_bias=np.zeros(3), accelerometer_bias=np.zeros(3))
    filt = SimpleNamespace(
        state=SimpleNamespace(cameras=OrderedDict(), covariance=z["P0"].copy(), imu=imu), K=z["K"], sigma_image=run.sigma,
        features=OrderedDict(), number_of_residuals_discarded_for_gasting_test=0, estimated_world_points=[],
        min_number_of_frames_to_be_lost=params.min_frames_lost, min_number_of_frames_to_be_tracked=params.min_frames_tracked,
        use_parallax=params.use_parallax, min_parallax=params.min_parallax_deg, last_camera_measurement=None,
        width=params.width, height=params.height)

    def remove_features(features):                   # MSCKF.py:739-749
        for fid in features:
            del filt.features[fid]
        seen = {ci for ft in filt.features.values() for ci in ft.camera_indices}
        filt.removed_by_features = [k for k in filt.state.cameras if k not in seen]
        _remove_cameras(filt, filt.removed_by_features)
    filt.remove_features = remove_features
    return filt


def _add_frame_views(run, filt, c, key):
    """This frame's views from the pool, appended as add_camera_measurements does (`MSCKF.py:403-438`)."""
    cams = filt.state.cameras
    cam = cams[key]
    vp = c["view_ptr"]
    seen = set()
    for j, fid in enumerate(c["ids"].tolist()):
        rows = [v for v in range(vp[j], vp[j + 1]) if int(c["obs_key"][v]) == key]
        if not rows:
            continue
        v = rows[0]
        line = SimpleNamespace(base=cam.T_W_Ci.t, direction=c["line_dir"][v], confidence=float(c["line_conf"][v]))
        if fid not in filt.features:                 # :420-434
            idp = SimpleNamespace(base=cam.T_W_Ci.t, m=c["idp_m"][j].copy(), rho=float(c["idp_rho"][j]))
            filt.features[fid] = SimpleNamespace(keypoints=[], descriptors=[], scores=[], camera_indices=[], lines=[],
                                                 inverse_depth_point=idp, tracked_for_n_frames=0, lost_for_n_frames=0)
        ft = filt.features[fid]
        ft.keypoints.append(c["obs_uv"][v].copy())
        ft.descriptors.append(None)
        ft.scores.append(float(c["line_conf"][v]))
        ft.camera_indices.append(key)
        ft.lines.append(line)
        ft.tracked_for_n_frames += 1
        ft.lost_for_n_frames = 0
        seen.add(fid)
    for fid, ft in filt.features.items():
        if fid not in seen:
            ft.lost_for_n_frames += 1                # :438


def _check_entry(filt, c):
    """The filter's own bookkeeping against what the reference held at the call's entry."""
    feats = filt.features if c["kind"] == PROCESS else None
    if feats is None:
        drop = {int(c["keys"][s]) for s in c["rm"]}
        feats = OrderedDict((i, ft) for i, ft in filt.features.items() if any(k in drop for k in ft.camera_indices))
    assert list(feats.keys()) == c["ids"].tolist()
    assert [len(ft.keypoints) for ft in feats.values()] == np.diff(c["view_ptr"]).tolist()
    cams = filt.state.cameras
    base = np.array([ln.base for ft in feats.values() for ln in ft.lines]).reshape(-1, 3)
    np.testing.assert_allclose(base, c["line_base"], rtol=0, atol=POSE_TOL)
    for ft in feats.values():
        for ln, ci in zip(ft.lines, ft.camera_indices):
            assert ln.base is cams[ci].T_W_Ci.t      # aliasing kept through every injection (inject.py, :661)
    np.testing.assert_allclose(np.array([ft.inverse_depth_point.base for ft in feats.values()]).reshape(-1, 3),
                               c["idp_base"], rtol=0, atol=POSE_TOL)
    np.testing.assert_allclose(np.array([ft.inverse_depth_point.m for ft in feats.values()]).reshape(-1, 3),
                               c["idp_m"], rtol=0, atol=TOL)
    np.testing.assert_allclose([ft.inverse_depth_point.rho for ft in feats.values()], c["idp_rho"], rtol=TOL)
    assert [ft.lost_for_n_frames for ft in feats.values()] == c["lost"].tolist()
    assert [ft.tracked_for_n_frames for ft in feats.values()] == c["tracked"].tolist()


def _check_exit(filt, c):
    assert list(filt.features.keys()) == c["exit_ids"].tolist()
    assert [len(ft.keypoints) for ft in filt.features.values()] == c["exit_nview"].tolist()


def _check_poses(filt, c):
    cams = list(filt.state.cameras.values())
    np.testing.assert_allclose(np.array([cm.T_W_Ci.R for cm in cams]), c["post_R"], rtol=0, atol=POSE_TOL)
    np.testing.assert_allclose(np.array([cm.T_W_Ci.t for cm in cams]), c["post_t"], rtol=0, atol=POSE_TOL)


def test_drop_in_window30_run_tracks_the_reference(run, eng):
    z = run.z
    filt = _make_filter(run)
    worst = dict(dx=0.0, probe=0.0)
    calls_of_frame = {}
    for o, (kind, idx) in enumerate(run.ops):
        if kind in (PROCESS, PRUNE):
            calls_of_frame.setdefault(run.call(idx)["frame"], []).append((o, kind, idx))
    remove_op = {int(idx): o for o, (kind, idx) in enumerate(run.ops) if kind == REMOVE}
    seen_dx = []
    eng_result = eng.result

    def result():                                        # process_features' own read-back, kept for the dx check
        res = eng_result()
        seen_dx.append(res.dx)
        return res
    eng.result = result
    try:
        _drop_in_frames(run, eng, filt, calls_of_frame, remove_op, seen_dx, worst)
    finally:
        del eng.result
    print(f"drop-in window30: worst dx {worst['dx']:.2e}, probes {worst['probe']:.2e}")


def _drop_in_frames(run, eng, filt, calls_of_frame, remove_op, seen_dx, worst):
    z = run.z
    o = 0
    frame = 0
    while o < len(run.ops):
        kind, idx = run.ops[o]
        if kind == IMU:                                  # the covariance steps either side: on the engine as well
            if o == 0 or run.ops[o - 1][0] != IMU:
                cams = filt.state.cameras
                eng.set_prior(filt.state.covariance, z["gravity"], z["K"], run.sigma,
                              [cm.T_W_Ci.R for cm in cams.values()], [cm.T_W_Ci.t for cm in cams.values()])
            _imu_step(run, eng, idx)
            if o in run.probes:
                _check_probe(run, o, eng.covariance(), worst)
        elif kind == AUGMENT:
            a = _augment(run, eng, idx)
            filt.state.covariance = eng.covariance()
            _check_probe(run, o, filt.state.covariance, worst)
            pose = SimpleNamespace(R=a["cam_R"].copy(), t=a["cam_t"].copy())
            key = int(a["key"])
            filt.state.cameras[key] = SimpleNamespace(T_W_Ci=pose, T_W_Ci_null=pose, width=filt.width, height=filt.height)
            for o2, k2, i2 in calls_of_frame[frame]:
                c = run.call(i2)
                if k2 == PROCESS:
                    _add_frame_views(run, filt, c, key)
                    _check_entry(filt, c)
                    filt.removed_by_features = []
                    seen_dx.clear()
                    status = eng.process_features(filt)
                    assert status == c["status"]
                    if status == 0:
                        e = rel_err(seen_dx[-1], c["dx"])
                        worst["dx"] = max(worst["dx"], e)
                        assert e < TOL, (o2, e)
                    if len(c["rm"]):
                        keys = c["keys"].tolist()
                        assert sorted(keys.index(k) for k in filt.removed_by_features) == c["rm"].tolist()
                        _check_probe(run, remove_op[i2], filt.state.covariance, worst)
                    else:
                        _check_poses(filt, c)
                        _check_probe(run, o2, filt.state.covariance, worst)
                    _check_exit(filt, c)
                else:
                    _check_entry(filt, c)
                    status = eng.prune_poorest_camera_states(filt)
                    assert status == c["status"]
                    assert list(filt.state.cameras.keys()) == [k for s, k in enumerate(c["keys"].tolist()) if s not in c["rm"]]
                    _check_poses(filt, c)
                    _check_probe(run, o2, filt.state.covariance, worst)
                    _check_exit(filt, c)
                    assert eng.n_clones == len(filt.state.cameras)
            frame += 1
        o += 1
    assert frame == len(z["aug_key"])
