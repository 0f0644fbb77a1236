"""CPU checks behind the resident nominal state (`msckf_set_nominal` ... `msckf_commit_inject`).

(a) The 30-clone fixture pins the nominal-state loop: integrating its samples as `IMU.integrate` does and injecting its
updates' `dx` as `inject.py` does reproduces every stored IMU state, augmentation pose and post-update clone pose.  This
guards the GPU test's own reconstruction of raw samples and biases (`nominal_ref.py`).
(b) The built library exports the new entry points and `_ffi` binds them with the documented argument types."""
import ctypes as C

import numpy as np
import pytest

import nominal_ref
import window30
from window30 import AUGMENT, IMU, PROCESS, PRUNE, REMOVE

REPLAY_TOL = 1e-12


@pytest.fixture(scope="module")
def run():
    return window30.Run()


def test_fixture_replay_reproduces_the_reference_nominal_state(run):
    from msckf_amd import inject, propagation
    z = run.z
    R, t, v = z["imu_R0"][0].copy(), z["imu_t0"][0].copy(), z["imu_v0"][0].copy()
    cam_R, cam_t = np.zeros((0, 3, 3)), np.zeros((0, 3))
    worst = 0.0

    def close(a, b):
        nonlocal worst
        e = float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.size(a) else 0.0
        worst = max(worst, e)
        assert e <= REPLAY_TOL, e

    n_imu = n_aug = n_upd = 0
    for kind, idx in run.ops:
        if kind == IMU:
            s = run.imu(idx)
            close(R, s["R0"]), close(t, s["t0"]), close(v, s["v0"])          # null state = state at entry, also after an update
            R, t, v, _ = nominal_ref.integrate(R, t, v, s["acc"], s["gyro"], float(s["dt"]), z["gravity"], s["w_planet"])
            close(R, s["R"]), close(t, s["t"]), close(v, s["v"])
            n_imu += 1
        elif kind == AUGMENT:
            a = run.aug(idx)
            close(R, a["imu_R"]), close(t, a["imu_t"])
            _, cR, ct = propagation.augmentation(R, t, (z["T_W_I_R"], z["T_W_I_t"]), (z["T_W_C_R"], z["T_W_C_t"]))
            close(cR, a["cam_R"]), close(ct, a["cam_t"])
            cam_R, cam_t = np.concatenate([cam_R, cR[None]]), np.concatenate([cam_t, ct[None]])
            n_aug += 1
        elif kind in (PROCESS, PRUNE):
            c = run.call(idx)
            if c["status"] == 0:
                dx = c["dx"]
                R = inject.corrected_rotation(R, dx[0:3])
                t, v = t + dx[12:15], v + dx[6:9]
                for i in range(len(cam_R)):
                    cam_R[i] = inject.corrected_rotation(cam_R[i], dx[15 + 6 * i:18 + 6 * i])
                    cam_t[i] = cam_t[i] + dx[18 + 6 * i:21 + 6 * i]
                n_upd += 1
            if kind == PRUNE:
                keep = [s for s in range(len(cam_R)) if s not in c["rm"]]
                cam_R, cam_t = cam_R[keep], cam_t[keep]
            close(cam_R, c["post_R"]), close(cam_t, c["post_t"])
        elif kind == REMOVE:
            c = run.call(idx)
            keep = [s for s in range(len(cam_R)) if s not in c["rm"]]
            cam_R, cam_t = cam_R[keep], cam_t[keep]
    assert (n_imu, n_aug) == (len(z["imu_dt"]), len(z["aug_key"])) and n_upd >= 40
    print(f"replay: {n_imu} samples, {n_aug} augmentations, {n_upd} updates, worst difference {worst:.1e}")


def test_raw_samples_and_biases_rebuild_the_stored_samples(run):
    bg, ba = nominal_ref.biases(run)
    gyro, acc = nominal_ref.raw_samples(run)
    assert np.any(bg != 0) and np.any(ba != 0)
    # one rounding of the sum, one of the difference: a few ulp of the sample
    assert np.max(np.abs((gyro - bg) - run.z["imu_gyro"])) <= 4 * np.finfo(float).eps * np.max(np.abs(gyro))
    assert np.max(np.abs((acc - ba) - run.z["imu_acc"])) <= 4 * np.finfo(float).eps * np.max(np.abs(acc))
    groups = [g for g in nominal_ref.imu_groups(run) if g[0] == "imu"]
    assert sum(len(g[1]) for g in groups) == len(run.z["imu_dt"]) and all(len(g[1]) == 4 for g in groups)


def test_nominal_entry_points_are_exported_and_bound(engine_lib):
    from msckf_amd import _ffi
    vp, dp = C.c_void_p, C.c_void_p
    want = {
        "msckf_set_nominal": [vp, C.POINTER(_ffi.NominalC)],
        "msckf_get_nominal": [vp, C.POINTER(_ffi.NominalC), dp, dp],
        "msckf_propagate_imu": [vp, C.c_int32, dp, dp, dp],
        "msckf_augment_imu": [vp],
        "msckf_commit_inject": [vp],
    }
    for name, argtypes in want.items():
        assert name in _ffi.SYMBOLS, name
        fn = getattr(engine_lib, name)
        assert fn.argtypes == argtypes and fn.restype is C.c_int, name
    # msckf_nominal: 198 doubles in the header's order
    assert C.sizeof(_ffi.NominalC) == 198 * 8
    assert [f[0] for f in _ffi.NominalC._fields_] == ["R", "t", "v", "b_g", "b_a", "R0", "t0", "v0", "gravity",
                                                       "planet_rate", "Qc", "T_I_C_R", "T_I_C_t"]
    assert _ffi.NominalC.Qc.offset == 42 * 8 and _ffi.NominalC.T_I_C_R.offset == 186 * 8
    assert _ffi.IMU_BATCH_MAX == 64
