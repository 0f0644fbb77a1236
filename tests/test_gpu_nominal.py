"""The nominal state resident beside the covariance: `set_nominal`, `propagate_imu`, `augment_imu`, `commit_inject`.

1-2  The reference's 30-clone run (`golden/window30/seq_window30.npz`) with the IMU state, biases and clone poses kept
     on the device: raw samples in (one call per frame, or split 1 + 3, or 4 x 1), no `propagate` / `augment` /
     `set_poses` and no host arithmetic in between.
3    Branches the run does not reach (planet rate, a zero-rate sample, unequal dt) against the host path
     `propagation.imu_transition` -> `propagate` on a second engine.
4    The injection alone against `inject.corrected_rotation`.
5    Call order, argument checks, no-op and failed updates.

Tolerances are the fixture's (`test_gpu_window30.py`): flags, masks, status and counters exact; dx, probes and
checkpoints 1e-8 relative with P exactly symmetric; poses, IMU state and biases 1e-9 absolute."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err
import nominal_ref
import window30
from window30 import AUGMENT, PROCESS, PRUNE, REMOVE
from test_gpu_select import EPS

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


@pytest.fixture(scope="module")
def eng_host():
    from msckf_amd.api import UpdateEngine
    e = UpdateEngine(max_clones=31, max_features=4096, max_track=31)
    yield e
    e.close()


def _close(a, b, what):
    e = float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.size(b) else 0.0
    assert np.shape(a) == np.shape(b) and e <= POSE_TOL, (what, e)
    return e


def _check_cov(run, o, eng, worst):
    if o in run.probes or o in run.checkpoints:
        P = eng.covariance()
        assert np.array_equal(P, P.T), o
        for ref, got in ((run.probes.get(o), lambda: P @ run.V[:P.shape[0]]), (run.checkpoints.get(o), lambda: P)):
            if ref is not None:
                e = rel_err(got(), ref)
                worst["probe"] = max(worst["probe"], e)
                assert e < TOL, (o, e)


def _check_selection(sel, exp_flags, exp_m, exp_rho, exp_world, cond):
    """`test_gpu_select.check_selection` where the poses are the engine's own.  Flags exact, unrefreshed points bit for
    bit, triangulated points (lines only) at that test's tolerance.  A refreshed point is the triangulated point seen from
    its anchor clone (`Camera.py:13-52`), m = R^T (X - t) / |.|, rho = 1 / |.|: with the pose within POSE_TOL of the
    reference's entry by entry (asserted after every update; a 3x3 of such entries has norm <= 3 POSE_TOL) m moves by at
    most |dR| + rho |dt| and rho by rho^2 |dt|: 3 POSE_TOL (1 + rho) on top of that test's own bound."""
    assert np.array_equal(sel.flags, exp_flags)
    tol = np.minimum(np.maximum(200 * EPS * cond, 1e-12), TOL)
    ref_mask = (exp_flags & 4) > 0
    pose = 3 * POSE_TOL * (1 + np.abs(exp_rho))
    assert np.all(np.abs(sel.idp_rho - exp_rho) <= (tol + pose) * np.abs(exp_rho))
    assert np.all(np.abs(sel.idp_m - exp_m).max(axis=1) <= tol + pose)
    scale = np.maximum(np.linalg.norm(exp_world[ref_mask], axis=1), 1.0)
    assert np.all(np.linalg.norm(sel.world[ref_mask] - exp_world[ref_mask], axis=1) <= tol[ref_mask] * scale)
    keep = ~ref_mask
    assert np.array_equal(sel.idp_rho[keep], exp_rho[keep]) and np.array_equal(sel.idp_m[keep], exp_m[keep])


SPLITS = {"whole": lambda g: [g], "1+3": lambda g: [g[:1], g[1:]], "4x1": lambda g: [[i] for i in g]}


@pytest.mark.parametrize("split", list(SPLITS))
def test_window30_run_with_the_nominal_state_resident(run, eng, split):
    from oracle import msckf_oracle as oracle
    z = run.z
    params = run.select_params()
    gyro, acc = nominal_ref.raw_samples(run)
    eng.set_prior(z["P0"], z["gravity"], z["K"], run.sigma)
    eng.set_nominal(z["imu_R0"][0], z["imu_t0"][0], z["imu_v0"][0], z["gravity"], z["Qc"],
                    T_W_I=(z["T_W_I_R"], z["T_W_I_t"]), T_W_C=(z["T_W_C_R"], z["T_W_C_t"]))
    keys = []
    b_g, b_a = np.zeros(3), np.zeros(3)
    worst = dict(dx=0.0, probe=0.0, state=0.0)
    split_updates = updates = 0
    groups = nominal_ref.imu_groups(run)
    for gi, (kind, idx, o) in enumerate(groups):
        if kind == "imu":
            for batch in SPLITS[split](idx):
                eng.propagate_imu(gyro[batch], acc[batch], z["imu_dt"][batch])      # raw samples, ONE call per batch
                s, last = eng.nominal(), batch[-1]
                for name in ("R", "t", "v"):
                    worst["state"] = max(worst["state"], _close(s[name], z["imu_" + name][last], (o, name)))
                    _close(s[name + "0"], z["imu_" + name][last], (o, name + "0"))   # MSCKF.py:247-248
                _close(s["b_g"], b_g, (o, "b_g")), _close(s["b_a"], b_a, (o, "b_a"))
                _check_cov(run, o - (idx[-1] - last), eng, worst)
            continue
        if kind == AUGMENT:
            a = run.aug(idx)
            eng.augment_imu()
            keys.append(int(a["key"]))
            s = eng.nominal()
            _close(s["cam_R"][-1], a["cam_R"], (o, "aug R")), _close(s["cam_t"][-1], a["cam_t"], (o, "aug t"))
        elif kind in (PROCESS, PRUNE):
            c = run.call(idx)
            assert c["keys"].tolist() == keys and eng.n_clones == len(keys)
            N = len(keys)
            held = eng.nominal()                             # (the oracle's conditioning estimate below reads the poses)
            prob = run.problem(c, np.zeros((15 + 6 * N,) * 2), held["cam_R"], held["cam_t"])
            tracks = run.tracks(c)
            eng.set_features(prob)                           # only the batch travels; P, poses and IMU state are resident
            eng.set_tracks(tracks)
            eng.run_select(params, prob.K)
            sel = eng.selection()
            cond = oracle.select_features(prob, tracks, params)["cond"]
            _check_selection(sel, c["flags"], c["sel_m"], c["sel_rho"], c["world"], cond)
            n_valid = int(sel.valid.sum())
            if 0 < n_valid < 0.15 * prob.F:
                eng.replan()
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
                    b_g, b_a = b_g + c["dx"][3:6], b_a + c["dx"][9:12]
                assert eng.commit_inject() == res.status
            else:
                assert c["status"] == 1
            if kind == PRUNE:
                eng.remove_clones(c["rm"])
                keys = [k for s, k in enumerate(keys) if s not in c["rm"]]
            s = eng.nominal()
            _close(s["cam_R"], c["post_R"], (o, "post R")), _close(s["cam_t"], c["post_t"], (o, "post t"))
            _close(s["b_g"], b_g, (o, "b_g")), _close(s["b_a"], b_a, (o, "b_a"))
            rest = [g for g in groups[gi + 1:] if g[0] in ("imu", PROCESS, PRUNE)]
            nxt = rest[0][1][0] if rest and rest[0][0] == "imu" else None
            if nxt is not None:                              # the frame's last injection: the IMU state is what the next sample starts from
                for name in ("R", "t", "v"):
                    _close(s[name], z["imu_" + name + "0"][nxt], (o, "injected " + name))
        elif kind == REMOVE:
            c = run.call(idx)
            before = eng.nominal()
            eng.remove_clones(c["rm"])
            keep = [s for s in range(len(keys)) if s not in c["rm"]]
            keys = [keys[s] for s in keep]
            s = eng.nominal()
            assert np.array_equal(s["cam_R"], before["cam_R"][keep]) and np.array_equal(s["cam_t"], before["cam_t"][keep])
        assert eng.n_clones == len(keys)
        _check_cov(run, o, eng, worst)
    assert split_updates >= 10, split_updates
    print(f"nominal window30 [{split}]: {updates} updates, {split_updates} with split long tracks; worst dx {worst['dx']:.2e}, "
          f"probes {worst['probe']:.2e}, IMU state {worst['state']:.2e}")


# ---- 3: branches the run does not reach ---------------------------------------------------------------------------
def _rot(axis, angle):
    from msckf_amd import inject
    return inject.corrected_rotation(np.eye(3), -np.asarray(axis, dtype=np.float64) * angle)


@pytest.mark.parametrize("N", [0, 1, 30])
def test_planet_rate_zero_rate_sample_and_unequal_dt_against_the_host_path(eng, eng_host, N):
    from msckf_amd import propagation
    rng = np.random.default_rng(40 + N)
    d = 15 + 6 * N
    A = rng.standard_normal((d, d))
    P0 = A @ A.T / d + np.eye(d) * 0.1
    P0 = 0.5 * (P0 + P0.T)
    cam_R = np.array([_rot(rng.standard_normal(3), 0.3) for _ in range(N)]).reshape(N, 3, 3)
    cam_t = rng.standard_normal((N, 3))
    gravity, K = np.array([0.0, 0.0, -9.81]), np.array([[400.0, 0, 320], [0, 400, 240], [0, 0, 1]])
    Qc = np.diag(np.repeat([1e-4, 1e-6, 1e-3, 1e-5], 3)) + 1e-7 * np.ones((12, 12))
    # a rotation about z, a planet rate along z and dyadic biases: R^T w_planet and raw - bias are exact, so the first
    # sample's rate is exactly zero on the host and on the device (IMU.py:89-90)
    w_planet = np.array([0.0, 0.0, 2.0 ** -13])
    b_g, b_a = np.array([0.25, -0.125, 0.5]) * 2.0 ** -6, np.array([0.03, -0.02, 0.05])
    c, s = np.cos(0.3), np.sin(0.3)
    R, t, v = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), rng.standard_normal(3), rng.standard_normal(3)
    n = 7
    gyro = rng.standard_normal((n, 3)) * 0.4 + b_g
    gyro[0] = w_planet + b_g
    acc = rng.standard_normal((n, 3)) * 2.0 + np.array([0.0, 0.0, 9.81])
    dt = np.array([0.005, 0.01, 0.0025, 0.005, 0.02, 0.001, 0.005])
    for e in (eng, eng_host):
        e.set_prior(P0, gravity, K, 0.2, cam_R, cam_t)
    eng.set_nominal(R, t, v, gravity, Qc, T_I_C=(np.eye(3), np.zeros(3)), b_g=b_g, b_a=b_a, planet_rate=w_planet)
    eng.propagate_imu(gyro, acc, dt)
    thetas = []
    for k in range(n):                                       # the host path, sample by sample
        g, a = gyro[k] - b_g, acc[k] - b_a
        R0, t0, v0 = R, t, v
        R, t, v, theta = nominal_ref.integrate(R, t, v, a, g, float(dt[k]), gravity, w_planet)
        thetas.append(theta)
        Phi, Q = propagation.imu_transition(R, t, v, R0, t0, v0, g, a, float(dt[k]), gravity, Qc, w_planet)
        eng_host.propagate(Phi, Q)
    assert thetas[0] == 0.0 and all(th > 0 for th in thetas[1:])
    got, P, Ph = eng.nominal(), eng.covariance(), eng_host.covariance()
    _close(got["R"], R, "R"), _close(got["t"], t, "t"), _close(got["v"], v, "v")
    _close(got["R0"], R, "R0"), _close(got["t0"], t, "t0"), _close(got["v0"], v, "v0")
    assert np.array_equal(got["b_g"], b_g) and np.array_equal(got["b_a"], b_a)
    assert np.array_equal(got["cam_R"], cam_R) and np.array_equal(got["cam_t"], cam_t)
    assert np.array_equal(P, P.T)
    e = rel_err(P, Ph)
    print(f"N = {N}: covariance against the host path {e:.2e}")
    assert e < TOL, e


# ---- 4: the injection alone -----------------------------------------------------------------------------------------
def test_injection_against_the_host_injection(eng):
    from msckf_amd import inject, synth
    rng = np.random.default_rng(7)
    N = 30
    prob = synth.make_problem(N, 200, 8, seed=11)
    off = lambda R: R + 1e-7 * rng.standard_normal(R.shape)          # as after many additive steps
    prob.cam_R = off(np.asarray(prob.cam_R, dtype=np.float64))
    prob.cam_R0 = prob.cam_R.copy()
    eng.load(prob)
    R, t, v = off(_rot([1.0, 2.0, -1.0], 0.2)), rng.standard_normal(3), rng.standard_normal(3)
    b_g, b_a = rng.standard_normal(3) * 0.01, rng.standard_normal(3) * 0.1
    eng.set_nominal(R, t, v, prob.gravity, np.eye(12), T_I_C=(np.eye(3), np.zeros(3)), b_g=b_g, b_a=b_a)
    eng.run()
    assert eng.result().status == 0
    # the dx the injection reads is the one in HBM: replace it by one that covers every branch
    mags = np.concatenate([[1e-12, 0.0, 5e-9, 2e-8, 1e-6], np.geomspace(1e-3, 0.5, N + 1 - 5)])   # IMU, then clone 0 ..
    dx = rng.standard_normal(15 + 6 * N) * 0.05
    for i, m in enumerate(mags):
        u = rng.standard_normal(3)
        lo = 0 if i == 0 else 15 + 6 * (i - 1)
        dx[lo:lo + 3] = m * u / np.linalg.norm(u)
    assert not dx[15:18].any()                                        # exactly zero: the isclose branch
    eng.comm_put(eng.device_pointer(0), dx)
    assert eng.commit_inject() == 0
    s = eng.nominal()
    worst = _close(s["R"], inject.corrected_rotation(R, dx[0:3]), "R")
    _close(s["t"], t + dx[12:15], "t"), _close(s["v"], v + dx[6:9], "v")
    _close(s["b_g"], b_g + dx[3:6], "b_g"), _close(s["b_a"], b_a + dx[9:12], "b_a")
    for i in range(N):
        dc = dx[15 + 6 * i:21 + 6 * i]
        worst = max(worst, _close(s["cam_R"][i], inject.corrected_rotation(prob.cam_R[i], dc[:3]), ("cam R", i)))
        _close(s["cam_t"][i], prob.cam_t[i] + dc[3:], ("cam t", i))
    orth = max(float(np.max(np.abs(Rm.T @ Rm - np.eye(3)))) for Rm in [s["R"], *s["cam_R"]])
    print(f"injection: rotations against the host {worst:.2e}, R^T R - I {orth:.2e}")
    assert orth < 1e-14, orth


# ---- 5: call order, arguments, no-op and failed updates ----------------------------------------------------------------
def test_calls_before_set_nominal_and_batch_size_limits():
    from msckf_amd import _ffi
    from msckf_amd.api import UpdateEngine
    one = np.zeros((1, 3))
    with UpdateEngine(max_clones=4, max_features=16, max_track=4) as e:
        with pytest.raises(_ffi.EngineError) as err:                 # needs set_state / set_prior first
            e.set_nominal(np.eye(3), np.zeros(3), np.zeros(3), [0, 0, -9.81], np.eye(12), T_I_C=(np.eye(3), np.zeros(3)))
        assert err.value.code == _ffi.ERR_STATE
        e.set_prior(np.eye(15), [0, 0, -9.81], np.eye(3), 0.2)
        for call in (e.nominal, lambda: e.propagate_imu(one, one, [0.01]), e.augment_imu, e.commit_inject):
            with pytest.raises(_ffi.EngineError) as err:
                call()
            assert err.value.code == _ffi.ERR_STATE
        e.set_nominal(np.eye(3), np.zeros(3), np.zeros(3), [0, 0, -9.81], np.eye(12) * 1e-4, T_I_C=(np.eye(3), np.zeros(3)))
        nmax = _ffi.IMU_BATCH_MAX
        for n in (0, nmax + 1):
            with pytest.raises(_ffi.EngineError) as err:
                e.propagate_imu(np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, 0.01))
            assert err.value.code == _ffi.ERR_ARG
        rng = np.random.default_rng(0)
        e.propagate_imu(rng.standard_normal((nmax, 3)) * 0.1, rng.standard_normal((nmax, 3)), np.full(nmax, 0.005))
        e.augment_imu()
        s, P = e.nominal(), e.covariance()
        assert P.shape == (21, 21) and np.array_equal(P, P.T) and np.all(np.isfinite(P))
        assert np.max(np.abs(s["R"].T @ s["R"] - np.eye(3))) < 1e-13 and np.array_equal(s["cam_R"][0], s["R"])


def test_commit_inject_after_a_no_op_update_changes_nothing(eng):
    prob, z = load_golden("edge_all_rejected")
    assert int(z["status"]) == 1
    eng.load(prob)
    eng.set_nominal(np.eye(3), np.ones(3), np.ones(3), prob.gravity, np.eye(12), T_I_C=(np.eye(3), np.zeros(3)), b_g=[1, 2, 3])
    before, P = eng.nominal(), eng.covariance()
    eng.run()
    assert eng.result().status == 1
    assert eng.commit_inject() == 1
    after = eng.nominal()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert np.array_equal(eng.covariance(), P)


def test_a_failed_update_leaves_the_nominal_state_untouched():
    """MSCKF_DEBUG_FAKE_TIMEOUT=1 makes the context's first streamed update read as timed out; a batch with split long
    tracks is not retried and returns ERR_HIP.  A child process, as the switch is read once."""
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import msckf_amd
from msckf_amd import _ffi, synth
from msckf_amd.api import UpdateEngine
p = synth.make_problem(14, 40, 14, seed=1, variable_tracks=True, min_track=2)
with UpdateEngine(max_clones=14, max_features=64, max_track=14) as e:
    e.load(p)
    e.set_nominal(np.eye(3), np.ones(3), np.ones(3), p.gravity, np.eye(12), T_I_C=(np.eye(3), np.zeros(3)), b_a=[1, 2, 3])
    before, P = e.nominal(), e.covariance()
    e.run()
    codes = []
    for call in (e.result, e.commit_inject):
        try:
            call()
            codes.append(0)
        except _ffi.EngineError as err:
            codes.append(err.code)
    after = e.nominal()
    same = all(np.array_equal(before[k], after[k]) for k in before) and np.array_equal(e.covariance(), P)
    print("split", e.debug_split()["long_tracks"], "codes", codes, "same", same, flush=True)
    print("FAILED_UPDATE_OK" if codes == [_ffi.ERR_HIP, _ffi.ERR_HIP] and same and e.debug_split()["long_tracks"] > 0 else "FAILED_UPDATE_BAD")
""" % ROOT
    env = dict(os.environ, MSCKF_DEBUG_FAKE_TIMEOUT="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert "FAILED_UPDATE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
