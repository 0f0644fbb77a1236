"""The 30-clone filter run of the reference (`golden/window30/seq_window30.npz`, loader `window30.py`) on the CPU: the
fixture's coverage, and the oracle carrying its OWN covariance through every op of the run -- IMU propagation,
augmentation, selection + update on the resident state, pruning, removal of clones -- pinned to the reference by the
probes P @ V after each op and by full checkpoints."""
import os

import numpy as np
import pytest

from conftest import rel_err
import window30
from window30 import AUGMENT, IMU, PROCESS, PRUNE, REMOVE

PROBE_TOL = 1e-9
DX_TOL = 1e-8


@pytest.fixture(scope="module")
def run():
    return window30.Run()


def test_window30_fixture_properties(run):
    """What the run is for: a full window pruned again and again, split long tracks, tracks with holes, both branches of
    update, no decision near its threshold; and the bookkeeping of every call is self-consistent."""
    assert os.path.getsize(window30.PATH) <= window30.SIZE_LIMIT
    p = window30.properties(run)
    window30.assert_properties(p)
    z = run.z
    assert z["pool_uv"].dtype == np.float32 and z["pool_score"].dtype == np.float32
    for i in range(run.n_calls()):
        c = run.call(i)
        ids, nview = c["ids"], np.diff(c["view_ptr"])
        assert len(set(ids.tolist())) == len(ids) and (nview >= 1).all()
        assert c["n_rejected"] == int(((c["flags"] & 1) > 0).sum() - c["accepted"].sum())
        assert not c["accepted"][(c["flags"] & 1) == 0].any()
        assert (c["status"] == 0) == (len(c["dx"]) > 0)


def _so3_post(cam_R, cam_t, dx):
    from oracle import msckf_oracle as oracle
    R = np.stack([oracle.so3_correction(cam_R[i], dx[15 + 6 * i:18 + 6 * i]) for i in range(len(cam_R))])
    return R, cam_t + dx[15:].reshape(-1, 6)[:, 3:]


def carry(run, setup="oracle", check=None):
    """Replays the run on the host with the oracle's arithmetic, from P0 alone.  `setup`: who builds Phi, Q and the
    augmentation Jacobian -- "oracle" or the package's own host code ("host", propagation.py).  Yields (op number, kind,
    P, extra) after every op; asserts selection, gate, dx and poses of every call on the way."""
    from msckf_amd import propagation
    from oracle import msckf_oracle as oracle
    z = run.z
    params = run.select_params()
    P = z["P0"].copy()
    keys, cam_R, cam_t = [], np.zeros((0, 3, 3)), np.zeros((0, 3))
    worst = dict(dx=0.0, probe=0.0)
    for o, (kind, idx) in enumerate(run.ops):
        if kind == IMU:
            s = run.imu(idx)
            if setup == "host":
                Phi, Q = propagation.imu_transition(s["R"], s["t"], s["v"], s["R0"], s["t0"], s["v0"], s["gyro"], s["acc"],
                                                    float(s["dt"]), z["gravity"], z["Qc"], s["w_planet"])
            else:
                Phi, Q = oracle.imu_transition(s["R"], s["t"], s["v"], s["R0"], s["t0"], s["v0"], s["gyro"], s["acc"],
                                               float(s["dt"]), z["gravity"], s["w_planet"], z["Qc"])
            P = oracle.propagate_covariance(P, Phi, Q)
        elif kind == AUGMENT:
            a = run.aug(idx)
            if setup == "host":
                J, cR, ct = propagation.augmentation(a["imu_R"], a["imu_t"], (z["T_W_I_R"], z["T_W_I_t"]), (z["T_W_C_R"], z["T_W_C_t"]))
            else:
                J, cR, ct = oracle.augmentation_jacobian(a["imu_R"], a["imu_t"], z["T_W_I_R"], z["T_W_I_t"], z["T_W_C_R"], z["T_W_C_t"])
            np.testing.assert_allclose(cR, a["cam_R"], atol=1e-14)
            np.testing.assert_allclose(ct, a["cam_t"], atol=1e-14)
            P = oracle.augment_covariance(P, J)
            keys.append(int(a["key"]))
            cam_R, cam_t = np.concatenate([cam_R, a["cam_R"][None]]), np.concatenate([cam_t, a["cam_t"][None]])
        elif kind in (PROCESS, PRUNE):
            c = run.call(idx)
            assert c["keys"].tolist() == keys
            if kind == PRUNE:
                poorest = window30.poorest_two(c["counts"])
                assert sorted(keys.index(k) for k in poorest) == c["rm"].tolist()
            # the bases the reference held: every line on its clone's current position (aliasing, MSCKF.py:410)
            assert np.array_equal(c["line_base"], cam_t[c["obs_slot"]])
            prob = run.problem(c, P, cam_R, cam_t)
            sel = oracle.select_features(prob, run.tracks(c), params)
            assert np.array_equal(sel["flags"], c["flags"])
            np.testing.assert_allclose(sel["idp_rho"], c["sel_rho"], rtol=1e-9)
            np.testing.assert_allclose(sel["idp_m"], c["sel_m"], rtol=0, atol=1e-9)
            valid = np.nonzero(c["flags"] & 1)[0]
            if len(valid):
                upd = prob.take(valid)
                upd.idp_m, upd.idp_rho = sel["idp_m"][valid], sel["idp_rho"][valid]
                out = oracle.update(upd)
                assert np.array_equal(out["accepted"], c["accepted"][valid])
                assert out["n_rejected"] == c["n_rejected"] and out["status"] == c["status"]
                if out["status"] == 0:
                    e = rel_err(out["dx"], c["dx"])
                    worst["dx"] = max(worst["dx"], e)
                    assert e < DX_TOL, (o, e)
                    P = out["P_new"]
                    R_post, t_post = _so3_post(cam_R, cam_t, out["dx"])
                    keep = [s for s in range(len(keys)) if kind == PROCESS or s not in c["rm"]]
                    np.testing.assert_allclose(R_post[keep], c["post_R"], rtol=0, atol=1e-9)
                    np.testing.assert_allclose(t_post[keep], c["post_t"], rtol=0, atol=1e-9)
            else:
                assert c["status"] == 1 and c["n_rejected"] == 0
            if kind == PROCESS:
                cam_R, cam_t = c["post_R"].copy(), c["post_t"].copy()
            else:
                P = oracle.remove_clones_covariance(P, c["rm"])
                keys = [k for s, k in enumerate(keys) if s not in c["rm"]]
                cam_R, cam_t = c["post_R"].copy(), c["post_t"].copy()
        elif kind == REMOVE:
            c = run.call(idx)
            P = oracle.remove_clones_covariance(P, c["rm"])
            keep = [s for s in range(len(keys)) if s not in c["rm"]]
            keys = [keys[s] for s in keep]
            cam_R, cam_t = cam_R[keep], cam_t[keep]
        assert P.shape[0] == 15 + 6 * len(keys)
        if o in run.probes:
            e = rel_err(P @ run.V[:P.shape[0]], run.probes[o])
            worst["probe"] = max(worst["probe"], e)
            assert e < PROBE_TOL, (o, kind, e)
        if o in run.checkpoints:
            assert rel_err(P, run.checkpoints[o]) < PROBE_TOL
    assert len(keys) == run.n_clones_after()[-1]
    return worst


def test_window30_oracle_carries_the_run(run):
    """The oracle's own covariance through all ~50 selections and updates of the run, the prunes and every IMU step:
    flags exact, refreshed points 1e-9, accepted masks exact, dx 1e-8, probes and checkpoints 1e-9."""
    worst = carry(run, "oracle")
    assert worst["probe"] < PROBE_TOL


def test_window30_host_setup_carries_the_run(run):
    """The same replay with Phi, Q and J built by the package's host code (propagation.py)."""
    worst = carry(run, "host")
    assert worst["probe"] < PROBE_TOL
