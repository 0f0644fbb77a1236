"""What the nominal-state tests share: `IMU.integrate` restated, and the 30-clone run's raw IMU samples and biases
rebuilt from the fixture (`golden/window30/seq_window30.npz` stores bias-corrected samples).  Not a conftest: imported
by name."""
import numpy as np

import window30
from window30 import IMU, PROCESS, PRUNE


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def integrate(R, t, v, acc, gyro, dt, gravity, w_planet):
    """`IMU.integrate` (reference `src/msckf/IMU.py:78-100`); `acc`, `gyro` bias-corrected.  Returns (R, t, v, theta)."""
    w = gyro - R.T @ w_planet                                         # :83
    theta = np.linalg.norm(w) * dt                                    # :84
    if theta > 0:                                                     # :85-88
        S = _skew(w / np.linalg.norm(w))
        Rd = np.eye(3) + np.sin(theta) * S + (1 - np.cos(theta)) * S @ S
    else:
        Rd = np.eye(3)                                                # :90
    a = R @ acc - gravity                                             # :94
    return R @ Rd, t + v * dt + 0.5 * a * dt ** 2, v + a * dt, theta  # :92, :96, :97


def biases(run):
    """Per IMU sample the biases the reference held when it processed it: the running sums of the updates' corrections
    (`MSCKF.py:639-640`), which start at zero.  Returns (b_g (n, 3), b_a (n, 3))."""
    n = len(run.z["imu_dt"])
    bg, ba = np.zeros((n, 3)), np.zeros((n, 3))
    g, a = np.zeros(3), np.zeros(3)
    for kind, idx in run.ops:
        if kind == IMU:
            bg[idx], ba[idx] = g, a
        elif kind in (PROCESS, PRUNE):
            c = run.call(idx)
            if c["status"] == 0:
                g, a = g + c["dx"][3:6], a + c["dx"][9:12]
    return bg, ba


def raw_samples(run):
    """(gyro, acc) as the sensor gave them: the stored samples plus the biases of their time (exact up to one rounding)."""
    bg, ba = biases(run)
    return run.z["imu_gyro"] + bg, run.z["imu_acc"] + ba


def imu_groups(run):
    """The ops as a list of ("imu", [sample indices of consecutive IMU ops], op index of the last) and (kind, idx, op)."""
    out = []
    for o, (kind, idx) in enumerate(run.ops):
        if kind == IMU:
            if out and out[-1][0] == "imu" and out[-1][2] == o - 1:
                out[-1] = ("imu", out[-1][1] + [idx], o)
            else:
                out.append(("imu", [idx], o))
        else:
            out.append((kind, idx, o))
    return out


__all__ = ["integrate", "biases", "raw_samples", "imu_groups", "window30"]
