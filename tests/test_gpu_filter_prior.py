"""Every update path and the resident kernels either side of it on filter-shaped priors (tests/filter_prior.py), judged in
covariance units.

  a  one update per path: the K6-K7 forms below 54 clones, the streamed K6-K7, the chain, long tracks on both sides of the
     split's limit, the K5 plan's boundaries
  b  the chain forced (MSCKF_GAIN_STREAM=0, a child process) where the default never takes it
  c  the prior built by the device: 663 propagate / augment launches from the 15 x 15 P0 up to 221 clones, an update on it,
     commit, remove every third clone, a second update
  d  the nominal state resident at 63 - 221 clones: propagate_imu / augment_imu against the host path, the injection and the
     pose compaction past lane 64

Every update is held to `check`: status and mask the oracle's, P+ bit-symmetric, rel_err on dx and P+ below 1e-8 as everywhere
else, and scaled_dx, scaled_P, update_term below the same 1e-8 -- BASELINE.json's tolerance applied to the new measures, set
before the engine was ever seen in them.  The inputs were conditioned on the CPU (tests/test_filter_prior.py): the reference
spread of every case is below 1e-12 in all of them.  Each check prints `FILTERPRIOR <case> e_dx e_P s_dx s_P u_P`; the worst per
family are in DESIGN.md section 5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_prior as fp
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-8
POSE_TOL = 1e-9
MAX_N = fp.MAX_N


def check(name, res, ref, prob, populated=True):
    e = fp.metrics(res.dx, res.P_new, ref, prob.P)
    print(f"FILTERPRIOR {name} " + " ".join(f"{x:.2e}" for x in e))
    assert res.status == ref["status"]
    assert np.array_equal(res.accepted, ref["accepted"])
    if populated:
        assert 0 < int(ref["accepted"].sum()) < prob.F                # both sides of the gate are populated
    if res.status == 0:
        assert np.array_equal(res.P_new, res.P_new.T)
    e_dx, e_P, s_dx, s_P, u_P = e
    assert e_dx < TOL and e_P < TOL, (e_dx, e_P)
    assert s_dx < TOL and s_P < TOL and u_P < TOL, (s_dx, s_P, u_P)


def _engine():
    from msckf_amd.api import UpdateEngine
    return UpdateEngine(max_clones=MAX_N, max_features=512, max_track=31)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_host():
    e = _engine()
    yield e
    e.close()


def _family(*families):
    return [n for n, c in fp.CASES.items() if c.family in families]


# ---- a. one update per path ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", _family("forms", "stream", "chain", "few", "plan"))
def test_update_on_the_filter_prior(eng, name):
    prob, ref = fp.problem(name)
    check(name, eng.update_problem(prob), ref, prob, populated=name not in fp.NO_ROWS + fp.ONE_SIDED)


@pytest.mark.parametrize("name", _family("long"))
def test_long_tracks_on_the_filter_prior(eng, name):
    """Tracks of 11 - 31 views: split into narrow blocks + dense remainder rows up to N = 64, unsplit to the merge tree past it."""
    prob, ref = fp.problem(name)
    res = eng.update_problem(prob)
    assert (eng.debug_split()["long_tracks"] > 0) == (prob.N <= 64)
    check(name, res, ref, prob)


# ---- b. the chain forced where the default never takes it ---------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import msckf_amd
from msckf_amd.api import UpdateEngine
import filter_prior as fp
out = {}
with UpdateEngine(max_clones=%(max_n)d, max_features=512, max_track=31) as e:
    for name in json.loads(%(names)r):
        prob, ref = fp.problem(name)
        r = e.update_problem(prob)
        m = fp.metrics(r.dx, r.P_new, ref, prob.P)
        out[name] = dict(status=int(r.status), ref_status=int(ref["status"]), acc=bool(np.array_equal(r.accepted, ref["accepted"])),
                         n_acc=int(ref["accepted"].sum()), F=int(prob.F), sym=bool(np.array_equal(r.P_new, r.P_new.T)),
                         metrics=[float(x) for x in m])
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def forced():
    code = CHILD % dict(root=ROOT, names=json.dumps(_family("forced")), max_n=MAX_N)
    env = dict(os.environ, MSCKF_GAIN_STREAM="0")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1][len("RESULT "):])


@pytest.mark.parametrize("name", _family("forced"))
def test_chain_forced_on_the_filter_prior(forced, name):
    """k_chol16 + k_solve_lds<1..3>, the blocked 2 x 2 gain, k_chol<512> + k_solve<NREG>: every solve dispatch of the chain, T full."""
    r = forced[name]
    e_dx, e_P, s_dx, s_P, u_P = r["metrics"]
    print(f"FILTERPRIOR {name} " + " ".join(f"{x:.2e}" for x in r["metrics"]))
    assert r["status"] == r["ref_status"] == 0 and r["acc"] and r["sym"], r
    assert 0 < r["n_acc"] < r["F"], r
    assert e_dx < TOL and e_P < TOL, r
    assert s_dx < TOL and s_P < TOL and u_P < TOL, r


# ---- c. the prior built by the device -----------------------------------------------------------------------------------------

def test_prior_built_by_the_device(eng):
    """The resident sequence at wide windows: k_propagate / k_augment from an empty window to the widest, read back at the
    widths where the update's paths change, then the update, the commit and the compaction on what the device built."""
    from oracle import msckf_oracle as oracle
    import test_gpu_wide_windows as ww
    P_np, cam_R, cam_t, ops, _ = fp.filter_prior(MAX_N)
    h = fp.head()
    eng.set_prior(h["P0"], h["gravity"], h["K"], float(h["sigma"]))
    assert eng.n_clones == 0
    for op in ops:
        if op[0] == "propagate":
            eng.propagate(op[1], op[2])
            continue
        eng.augment(op[1], op[2], op[3])
        n = eng.n_clones
        if n in fp.KEPT:
            got, ref = eng.covariance(), fp.on_the_way(MAX_N, n)
            e, s = rel_err(got, ref), fp.scaled_P(got, ref)
            print(f"FILTERPRIOR device_built_{n} rel_err {e:.2e} scaled_P {s:.2e}")
            assert got.shape == ref.shape and np.array_equal(got, got.T), n
            assert e < 1e-10 and s < TOL, (n, e, s)
    assert eng.n_clones == MAX_N
    prob, ref = fp.problem("device_221")                               # built on NumPy's P, on the poses the device holds
    assert np.array_equal(prob.P, P_np) and np.array_equal(prob.cam_R, cam_R)
    eng.set_features(prob)
    eng.run()
    check("device_221", eng.result(), ref, prob)
    assert eng.commit_covariance() == 0
    P_c = eng.covariance()
    slots = list(range(0, MAX_N, 3))
    eng.remove_clones(slots)
    P_r = eng.covariance()
    assert eng.n_clones == MAX_N - len(slots) == 147
    assert np.array_equal(P_r, oracle.remove_clones_covariance(P_c, slots))       # a pure gather: bit-exact
    keep = [i for i in range(MAX_N) if i not in slots]
    batch = ww.full_problem(147, fp.SEED_BASE["device"] + 147, P=P_r, poses=(cam_R[keep], cam_t[keep]))
    eng.set_features(batch)
    eng.run()
    check("device_147_after_remove", eng.result(), oracle.update(batch, dense_noise=False), batch)


# ---- d. the nominal state resident at wide windows ----------------------------------------------------------------------------

def _close(a, b, what):
    e = float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.size(b) else 0.0
    assert np.shape(a) == np.shape(b) and e <= POSE_TOL, (what, e)
    return e


def _frames(h):
    return dict(T_W_I=(h["T_W_I_R"], h["T_W_I_t"]), T_W_C=(h["T_W_C_R"], h["T_W_C_t"]))


@pytest.mark.parametrize("N", [63, 64, 65, 221])
def test_nominal_state_resident_at_wide_windows(eng, eng_host, N):
    """k_propagate_imu / k_propagate_strip (up to 83 column tiles) in batches of 1, 3 and 64 samples and k_augment_imu against
    the host path `propagation.imu_transition` -> `propagate`, `propagation.augmentation` -> `augment` on a second engine."""
    from msckf_amd import propagation
    import nominal_ref
    P, cam_R, cam_t, _, imu = fp.filter_prior(N)
    h = fp.head()
    g, Qc, sigma = np.asarray(h["gravity"], dtype=np.float64), h["Qc"], float(h["sigma"])
    for e in (eng, eng_host):
        e.set_prior(P, g, h["K"], sigma, cam_R, cam_t)
    R, t, v = imu[-1]["R"], imu[-1]["t"], imu[-1]["v"]
    eng.set_nominal(R, t, v, g, Qc, **_frames(h))
    gyro = np.array([s["gyro"] for s in imu[:68]])
    acc = np.array([s["acc"] for s in imu[:68]])
    dt = np.full(68, 0.005)
    zero = np.zeros(3)
    k = 0
    for n in (1, 3, 64):
        eng.propagate_imu(gyro[k:k + n], acc[k:k + n], dt[k:k + n])           # raw samples, ONE call per batch
        for i in range(k, k + n):                                              # the host path, sample by sample
            R0, t0, v0 = R, t, v
            R, t, v, _ = nominal_ref.integrate(R, t, v, acc[i], gyro[i], float(dt[i]), g, zero)
            Phi, Q = propagation.imu_transition(R, t, v, R0, t0, v0, gyro[i], acc[i], float(dt[i]), g, Qc)
            eng_host.propagate(Phi, Q)
        k += n
        got = eng.nominal()
        _close(got["R"], R, "R"), _close(got["t"], t, "t"), _close(got["v"], v, "v")
        _close(got["R0"], R, "R0"), _close(got["t0"], t, "t0"), _close(got["v0"], v, "v0")
        assert np.array_equal(got["cam_R"], cam_R) and np.array_equal(got["cam_t"], cam_t)
    if N < MAX_N:
        eng.augment_imu()
        J, cR, ct = propagation.augmentation(R, t, *_frames(h).values())
        eng_host.augment(J, cR, ct)
        got = eng.nominal()
        _close(got["cam_R"][-1], cR, "aug R"), _close(got["cam_t"][-1], ct, "aug t")
        assert np.array_equal(got["cam_R"][:-1], cam_R) and np.array_equal(got["cam_t"][:-1], cam_t)
    Pd, Ph = eng.covariance(), eng_host.covariance()
    e, s = rel_err(Pd, Ph), fp.scaled_P(Pd, Ph)
    print(f"FILTERPRIOR nominal_{N} rel_err {e:.2e} scaled_P {s:.2e}")
    assert Pd.shape == Ph.shape and np.array_equal(Pd, Pd.T)
    assert e < TOL and s < TOL, (e, s)


def _rot(axis, angle):
    from msckf_amd import inject
    return inject.corrected_rotation(np.eye(3), -np.asarray(axis, dtype=np.float64) * angle)


@pytest.mark.parametrize("propagated", [False, True], ids=["null_apart", "null_aliased"])
@pytest.mark.parametrize("N", [64, 65, 221])
def test_injection_and_compaction_past_lane_64(eng, N, propagated):
    """k_inject's second workgroup (lane 64 is clone 63) and k_compact_poses' dynamic LDS beyond 31 poses.  The null state
    R0 / t0 / v0 moves with the state if and only if propagate_imu has run (NOM_ALIAS, MSCKF.py:247-248)."""
    from msckf_amd import inject
    from oracle import msckf_oracle as oracle
    name = f"inject_{N}"
    prob, ref = fp.problem(name)
    imu = fp.filter_prior(N)[4]
    h = fp.head()
    rng = np.random.default_rng(900 + N)
    off = lambda R: R + 1e-7 * rng.standard_normal(R.shape)          # as after many additive steps
    eng.set_state(prob)
    R, t, v = off(imu[-1]["R"]), imu[-1]["t"], imu[-1]["v"]
    R0, t0, v0 = _rot([1.0, -2.0, 0.5], 0.01) @ R, t + 0.01, v - 0.02
    b_g, b_a = rng.standard_normal(3) * 0.01, rng.standard_normal(3) * 0.1
    eng.set_nominal(R, t, v, prob.gravity, h["Qc"], b_g=b_g, b_a=b_a, R0=R0, t0=t0, v0=v0, **_frames(h))
    if propagated:
        eng.propagate_imu(imu[0]["gyro"][None] + b_g, imu[0]["acc"][None] + b_a, [0.005])
    eng.set_features(prob)
    eng.run()
    res = eng.result()
    if propagated:
        assert res.status == 0
    else:
        check(name, res, ref, prob)
    base = eng.nominal()
    if propagated:
        for k in "Rtv":
            assert np.array_equal(base[k + "0"], base[k])            # the reference holds ONE object as state and null state
    else:
        assert np.array_equal(base["R0"], R0) and np.array_equal(base["t0"], t0) and np.array_equal(base["v0"], v0)
    assert np.array_equal(base["cam_R"], prob.cam_R) and np.array_equal(base["cam_t"], prob.cam_t)
    # the dx the injection reads is the one in HBM: replace it by one whose rotations cover the isclose branch (|dtheta| <= 1e-8)
    # for the IMU and for clones on both sides of lane 64.  Item 0 is the IMU, item 1 + i clone i.
    mags = np.geomspace(1e-3, 0.5, N + 1)
    mags[:4] = [1e-12, 0.0, 5e-9, 2e-8]
    edge = [1e-6, 0.0, 1e-12, 5e-9, 2e-8, 1e-6]                      # items 61 .. 66: clones 60 .. 65, lane 64 = clone 63
    for item, m in zip(range(61, min(N + 1, 67)), edge):
        mags[item] = m
    dx = rng.standard_normal(15 + 6 * N) * 0.05
    for i, m in enumerate(mags):
        u = rng.standard_normal(3)
        lo = 0 if i == 0 else 15 + 6 * (i - 1)
        dx[lo:lo + 3] = m * u / np.linalg.norm(u)
    assert not dx[15:18].any() and not dx[15 + 6 * 61:18 + 6 * 61].any()       # exactly zero: clone 0 and clone 61
    eng.comm_put(eng.device_pointer(0), dx)
    assert eng.commit_inject() == 0
    s = eng.nominal()
    new_R = inject.corrected_rotation(base["R"], dx[0:3])
    worst = _close(s["R"], new_R, "R")
    _close(s["t"], base["t"] + dx[12:15], "t"), _close(s["v"], base["v"] + dx[6:9], "v")
    _close(s["b_g"], b_g + dx[3:6], "b_g"), _close(s["b_a"], b_a + dx[9:12], "b_a")
    if propagated:
        for k in "Rtv":
            assert np.array_equal(s[k + "0"], s[k]), k               # moved with the state
    else:
        assert np.array_equal(s["R0"], R0) and np.array_equal(s["t0"], t0) and np.array_equal(s["v0"], v0)
    for i in range(N):
        dc = dx[15 + 6 * i:21 + 6 * i]
        worst = max(worst, _close(s["cam_R"][i], inject.corrected_rotation(prob.cam_R[i], dc[:3]), ("cam R", i)))
        _close(s["cam_t"][i], prob.cam_t[i] + dc[3:], ("cam t", i))
    orth = max(float(np.max(np.abs(Rm.T @ Rm - np.eye(3)))) for Rm in [s["R"], *s["cam_R"]])
    print(f"FILTERPRIOR injection_{N} rotations against the host {worst:.2e}, R^T R - I {orth:.2e}")
    assert orth < 1e-14, orth
    slots = sorted({i for i in (0, 63, 64, N - 1) if i < N})
    P_c = eng.covariance()
    eng.remove_clones(slots)
    keep = [i for i in range(N) if i not in slots]
    after = eng.nominal()
    assert eng.n_clones == len(keep)
    assert np.array_equal(after["cam_R"], s["cam_R"][keep]) and np.array_equal(after["cam_t"], s["cam_t"][keep])
    assert np.array_equal(eng.covariance(), oracle.remove_clones_covariance(P_c, slots))
