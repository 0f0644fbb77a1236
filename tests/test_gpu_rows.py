"""Direct measurement rows on the resident filter (msckf_run_rows, msckf_run_fix, msckf_get_rows_gate; csrc/k_rows.h) against
the NumPy statement of the reference's update algebra in tests/rows_ref.py, on filter-shaped priors.

rel_err on dx and P+, scaled_dx, scaled_P and update_term stay below 1e-8 -- BASELINE.json's fp64 tolerance, applied as
tests/test_gpu_filter_prior.py applies it; tests/test_rows_ref.py holds every case's reference spread to 1e-12.  The kernels
are always fp64, so an MSCKF_DTYPE_F32 engine is held to the same number.  Every error in here is the return code of a
finished launch.
"""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import filter_prior as fp
import rows_ref as rr
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-8              # BASELINE.json, fp64
SAME = 1e-12            # two ways of giving the engine the same measurement
POSE_TOL = 1e-9         # tests/test_gpu_filter_prior.py

_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def engine(N, dtype="f64"):
    """One engine per window size (and dtype)."""
    from msckf_amd.api import UpdateEngine
    if (N, dtype) not in _engines:
        _engines[(N, dtype)] = UpdateEngine(max_clones=max(N, 1), max_features=128, max_track=10, dtype=dtype)
    return _engines[(N, dtype)]


def load(N, dtype="f64"):
    """The engine of N clones holding filter_prior(N) again."""
    eng = engine(N, dtype)
    P, cam_R, cam_t, _, _ = fp.filter_prior(N)
    h = fp.head()
    eng.set_prior(P, np.asarray(h["gravity"], dtype=np.float64), h["K"], float(h["sigma"]), cam_R, cam_t)
    return eng


def set_nominal(eng, N, b_g=None, b_a=None):
    h = fp.head()
    s = fp.filter_prior(max(N, 1))[4][-1]
    eng.set_nominal(s["R"], s["t"], s["v"], np.asarray(h["gravity"], dtype=np.float64), h["Qc"], b_g=b_g, b_a=b_a,
                    T_W_I=(h["T_W_I_R"], h["T_W_I_t"]), T_W_C=(h["T_W_C_R"], h["T_W_C_t"]))
    return s


def gate_arg(case, crit):
    return False if crit is None else True if case.gate == "table" else crit


def check(name, res, ref, P):
    e = fp.metrics(res.dx, res.P_new, ref, P)
    print(f"ROWS {name} " + " ".join(f"{x:.2e}" for x in e))
    assert res.status == ref["status"]
    assert res.accepted.shape == (1,) and bool(res.accepted[0]) == ref["applied"]
    assert np.array_equal(res.P_new, res.P_new.T)
    assert max(e) < TOL, e
    return e


def same(a, b, P, tol=SAME):
    e = fp.metrics(a.dx, a.P_new, dict(dx=b.dx, P_new=b.P_new), P)
    assert a.status == b.status and max(e) <= tol, e


def code(call):
    from msckf_amd import _ffi
    with pytest.raises(_ffi.EngineError) as e:
        call()
    return e.value.code


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rr.CASES))
def test_parity(name):
    case = rr.CASES[name]
    (P, H, r, R), crit, ref = rr.problem(name)
    eng = load(case.N)
    res = eng.update_rows(H, r, R, gate=gate_arg(case, crit))
    check(name, res, ref, P)
    again = eng.update_rows(H, r, R, gate=gate_arg(case, crit))
    assert np.array_equal(again.dx, res.dx) and np.array_equal(again.P_new, res.P_new)      # the same bits
    st = res.stats
    assert (st["n_features"], st["n_accepted"], st["n_rejected"], st["stacked_rows"]) == (1, int(ref["applied"]), int(not ref["applied"]), case.m)
    assert st["n_leaves"] == st["n_levels"] == st["k5_launches"] == st["not_spd"] == 0


def test_zero_clones():
    """N = 0: the standstill before the first clone, one ragged 15 x 15 tile."""
    for name in ("zupt_N0", "imu_17_N0"):
        (P, H, r, R), _, ref = rr.problem(name)
        eng = load(0)
        assert eng.covariance().shape == (15, 15)
        check(name + "_again", eng.update_rows(H, r, R), ref, P)
        assert eng.commit_covariance() == 0
        assert np.array_equal(eng.covariance(), eng.result().P_new)


def test_f32_context():
    (P, H, r, R), _, ref = rr.problem("dense_17_N30")
    eng = load(30, "f32")
    check("dense_17_N30_f32ctx", eng.update_rows(H, r, R), ref, P)


# ---- n_cols -------------------------------------------------------------------------------------------------------------------

def test_n_cols():
    (P, H, r, R), _, ref = rr.problem("imu_17_N30")
    eng = load(30)
    narrow = eng.update_rows(H, r, R)                                   # m x 15
    wide = eng.update_rows(rr.pad(H, P.shape[0]), r, R)                 # m x d, zero-padded
    same(narrow, wide, P)
    check("imu_17_N30_padded", wide, ref, P)
    # zero beyond column 8: m x 9, m x 15 and m x d
    H9 = np.array(H[:, :9])
    ref9 = rr.update(P, H9, r, R)
    got = [eng.update_rows(h, r, R) for h in (H9, rr.pad(H9, 15), rr.pad(H9, P.shape[0]))]
    same(got[0], got[1], P), same(got[0], got[2], P)
    check("imu_17_N30_9cols", got[0], ref9, P)
    # one column, one row: the narrowest call
    one = eng.update_rows(np.array([[1.0]]), np.array([1e-4]), 1e-3)
    check("one_by_one", one, rr.update(P, np.array([[1.0]]), np.array([1e-4]), np.array([[1e-6]])), P)


# ---- gate ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stem", ["imu_6_N30", "dense_17_N30"])
def test_gate_both_sides(stem):
    from msckf_amd import _ffi
    for side in ("above", "below"):
        name = f"{stem}_{side}"
        (P, H, r, R), crit, ref = rr.problem(name)
        eng = load(30)
        eng.run_rows(H, r, R, gate=crit)
        gamma, applied = eng.rows_gate()
        assert abs(gamma - ref["gamma"]) <= 1e-10 * ref["gamma"] and applied == ref["applied"] == (side == "above")
        res = eng.result()
        check(name + "_gate", res, ref, P)
        if side == "above":
            assert res.status == _ffi.OK and eng.commit_covariance() == _ffi.OK
            assert np.array_equal(eng.covariance(), res.P_new)
        else:
            assert res.status == _ffi.NOOP and not res.dx.any() and np.array_equal(res.P_new, P)
            assert eng.commit_covariance() == _ffi.NOOP
            assert np.array_equal(eng.covariance(), P)
            eng.run_rows(H, r, R, gate=crit)                             # ... and without result() in between
            assert eng.commit_covariance() == _ffi.NOOP and np.array_equal(eng.covariance(), P)


def test_gate_true_is_the_tables_entry():
    from msckf_amd.api import chi2_table
    (P, H, r, R), _, free = rr.problem("imu_15_N30")
    m = r.size
    eng = load(30)
    for factor, applied in ((1 - 1e-3, True), (1 + 1e-3, False)):
        rs = r * np.sqrt(factor * chi2_table()[m] / free["gamma"])      # gamma = factor * the table's entry for m rows
        ref = rr.update(P, H, rs, R, float(chi2_table()[m]))
        assert ref["applied"] == applied
        res = eng.update_rows(H, rs, R, gate=True)
        check(f"imu_15_N30_table_{factor:.3f}", res, ref, P)
        gamma, verdict = eng.rows_gate()
        assert verdict == applied and abs(gamma - ref["gamma"]) <= 1e-10 * ref["gamma"]


def test_nan_residual_is_rejected():
    from msckf_amd import _ffi
    (P, H, r, R), _, _ = rr.problem("imu_6_N30")
    bad = np.array(r)
    bad[2] = np.nan
    eng = load(30)
    for gate in (False, True, 1e300):
        res = eng.update_rows(H, bad, R, gate=gate)
        assert res.status == _ffi.NOOP and not res.dx.any() and np.array_equal(res.P_new, P)
        gamma, applied = eng.rows_gate()
        assert np.isnan(gamma) and not applied
        assert eng.commit_covariance() == _ffi.NOOP and np.array_equal(eng.covariance(), P)


# ---- not SPD, argument and state errors -----------------------------------------------------------------------------------------

def test_not_spd_and_errors():
    from msckf_amd import _ffi
    from msckf_amd.api import UpdateEngine
    (P, H, r, R), _, _ = rr.problem("imu_6_N30")
    d = P.shape[0]
    Hd = rr.pad(H, d)
    S0 = Hd @ P @ Hd.T
    R_bad = -(S0 + S0.T) / 2 - np.eye(r.size)
    H_nan = np.array(H)
    H_nan[1, 4] = np.nan
    eng = load(30)
    set_nominal(eng, 30)
    nominal = eng.nominal()
    for what, (h, rn) in dict(indefinite=(H, R_bad), nan_H=(H_nan, R), nan_R=(H, np.full_like(R, np.nan))).items():
        eng.run_rows(h, r, rn)
        assert code(eng.result) == _ffi.ERR_NOT_SPD, what
        eng.run_rows(h, r, rn)
        assert code(eng.commit_covariance) == _ffi.ERR_NOT_SPD, what
        eng.run_rows(h, r, rn)
        assert code(eng.commit_inject) == _ffi.ERR_NOT_SPD, what
        gamma, applied = eng.rows_gate()
        assert np.isnan(gamma) and not applied
        assert np.array_equal(eng.covariance(), P)
        after = eng.nominal()
        assert all(np.array_equal(after[k], nominal[k]) for k in nominal)
    # a sound update still goes through afterwards
    check("imu_6_N30_after_errors", eng.update_rows(H, r, R), rr.problem("imu_6_N30")[2], P)
    R_asym = np.array(R)
    R_asym[0, 1] = np.nextafter(R_asym[0, 1], 1.0)
    assert code(lambda: eng.run_rows(H, r, R_asym)) == _ffi.ERR_ARG
    assert code(lambda: eng.run_rows(np.zeros((0, 15)), np.zeros(0), np.zeros((0, 0)))) == _ffi.ERR_ARG
    assert code(lambda: eng.run_rows(np.ones((33, 15)), np.zeros(33), 1.0)) == _ffi.ERR_ARG
    assert code(lambda: eng.run_rows(np.ones((2, d + 1)), np.zeros(2), 1.0)) == _ffi.ERR_ARG
    assert eng._lib.msckf_run_rows(eng._h, 3, 15, None, _ffi.dptr(np.zeros(3)), _ffi.dptr(np.eye(3)), 0.0) == _ffi.ERR_ARG
    assert eng._lib.msckf_run_fix(eng._h, 3, _ffi.dptr(np.zeros(3)), _ffi.dptr(np.eye(3)), 0.0) == _ffi.ERR_ARG
    # (the refused calls launched nothing: the last run is still the sound one)
    assert eng.result().status == 0
    with UpdateEngine(max_clones=1, max_features=16, max_track=4) as fresh:
        assert code(lambda: fresh.run_rows(np.ones((1, 15)), np.zeros(1), 1.0)) == _ffi.ERR_STATE
        assert code(lambda: fresh.zero_velocity(0.1)) == _ffi.ERR_STATE
        assert code(fresh.rows_gate) == _ffi.ERR_STATE
    with UpdateEngine(max_clones=1, max_features=16, max_track=4) as e2:           # a state, but no nominal record
        P1, cR, ct, _, _ = fp.filter_prior(1)
        h = fp.head()
        e2.set_prior(P1, np.asarray(h["gravity"], dtype=np.float64), h["K"], float(h["sigma"]), cR, ct)
        assert code(lambda: e2.zero_velocity(0.1)) == _ffi.ERR_STATE
        e2.run_rows(np.ones((1, 15)), np.zeros(1), 1.0)                             # ... which rows of the caller do not need
        assert e2.result().status == 0


# ---- the fixes on the resident nominal state ----------------------------------------------------------------------------------

def _inject(nom, cam_R, cam_t, dx):
    """inject.inject_state on a state shaped like the reference's."""
    from msckf_amd import inject
    pose = lambda R, t: SimpleNamespace(R=np.array(R), t=np.array(t))
    imu = SimpleNamespace(T_W_Ii=pose(nom["R"], nom["t"]), v_W_Ii=np.array(nom["v"]), gyroscope_bias=np.array(nom["b_g"]),
                          accelerometer_bias=np.array(nom["b_a"]))
    cams = {i: SimpleNamespace(T_W_Ci=pose(cam_R[i], cam_t[i])) for i in range(len(cam_R))}
    state = SimpleNamespace(imu=imu, cameras=cams)
    inject.inject_state(state, dx)
    return state


@pytest.mark.parametrize("N", [3, 30])
def test_fixes_on_the_resident_nominal_state(N):
    import nominal_ref
    P0, cam_R, cam_t, _, imu = fp.filter_prior(N)
    h = fp.head()
    g = np.asarray(h["gravity"], dtype=np.float64)
    rng = np.random.default_rng(25000 + N)
    for which in ("zero_velocity", "velocity_fix", "position_fix"):
        eng = load(N)
        s0 = set_nominal(eng, N)
        n = 5
        gyro, acc, dt = np.array([s["gyro"] for s in imu[:n]]), np.array([s["acc"] for s in imu[:n]]), np.full(n, 0.005)
        eng.propagate_imu(gyro, acc, dt)                                 # pending: nothing is read back before the fix
        R, t, v = s0["R"], s0["t"], s0["v"]
        for i in range(n):
            R, t, v, _ = nominal_ref.integrate(R, t, v, acc[i], gyro[i], float(dt[i]), g, np.zeros(3))
        c0, nominal_value = (12, t) if which == "position_fix" else (6, v)
        sig = np.sqrt(np.diag(P0))[c0:c0 + 3]
        Rm = np.diag((0.5 * sig) ** 2) if which == "zero_velocity" else rr._full_noise(rng, sig, 0.5)
        Rm = (Rm + Rm.T) / 2
        z = np.zeros(3) if which == "zero_velocity" else nominal_value + 0.7 * sig * rng.standard_normal(3)
        if which == "zero_velocity":
            eng.zero_velocity(0.5 * sig)
        else:
            getattr(eng, which)(z, Rm)
        fix = eng.result()
        assert fix.status == 0
        Hs = np.zeros((3, c0 + 3))
        Hs[:, c0:] = np.eye(3)
        rows = eng.update_rows(Hs, z - nominal_value, Rm)                # the host-formed r = z - nominal, on the same P
        P = eng.covariance()                                            # (the propagated prior both ran on)
        same(fix, rows, P)
        ref = rr.update(P, Hs, z - nominal_value, Rm)
        check(f"{which}_N{N}", fix, ref, P)
        # the injection of that dx
        getattr(eng, which)(*((0.5 * sig,) if which == "zero_velocity" else (z, Rm)))
        before = eng.nominal()
        assert eng.commit_inject() == 0
        after = eng.nominal()
        st = _inject(before, before["cam_R"], before["cam_t"], ref["dx"])
        worst = 0.0
        for got, want in ((after["R"], st.imu.T_W_Ii.R), (after["t"], st.imu.T_W_Ii.t), (after["v"], st.imu.v_W_Ii),
                          (after["b_g"], st.imu.gyroscope_bias), (after["b_a"], st.imu.accelerometer_bias),
                          *((after["cam_R"][i], st.cameras[i].T_W_Ci.R) for i in range(N)),
                          *((after["cam_t"][i], st.cameras[i].T_W_Ci.t) for i in range(N))):
            worst = max(worst, float(np.max(np.abs(got - want))))
        print(f"ROWS {which}_N{N} injection against inject_state {worst:.2e}")
        assert worst <= POSE_TOL
        assert np.array_equal(eng.covariance(), fix.P_new)


def test_position_fix_sign_convention():
    """A position fix a million times tighter than the prior puts t on z: r = z - nominal, not the other way round."""
    N = 3
    eng = load(N)
    s0 = set_nominal(eng, N)
    sig = np.sqrt(np.diag(fp.filter_prior(N)[0]))[12:15]
    z = s0["t"] + np.array([0.8, -0.6, 0.4]) * sig
    eng.position_fix(z, 1e-6 * sig)
    assert eng.commit_inject() == 0
    t = eng.nominal()["t"]
    assert np.all(np.abs(t - z) <= 1e-5 * sig), (t - z) / sig
    # ... and a velocity fix likewise
    sv = np.sqrt(np.diag(eng.covariance()))[6:9]
    zv = eng.nominal()["v"] + np.array([-0.5, 0.7, 0.3]) * sv
    eng.velocity_fix(zv, 1e-6 * sv)
    assert eng.commit_inject() == 0
    assert np.all(np.abs(eng.nominal()["v"] - zv) <= 1e-5 * sv)


# ---- beside a camera batch ------------------------------------------------------------------------------------------------------

def test_beside_a_camera_batch():
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    prob, cam_ref = fp.problem("forms_10")
    zupt = rr.Case("zupt_N10", "zupt", 10, 3, None)
    _, H, _, _ = rr.measurement(zupt)
    with UpdateEngine(max_clones=10, max_features=128, max_track=10) as eng:
        # rows first, the camera batch already loaded: the batch survives and runs on the new P
        eng.set_state(prob)
        eng.set_features(prob)
        P, _, r, R = rr.measurement(zupt)
        assert np.array_equal(P, prob.P)
        rows_ref = rr.update(P, H, r, R)
        eng.run_rows(H, r, R)
        assert eng.commit_covariance() == 0
        eng.run()
        res = eng.result()
        want = oracle.update(dataclasses.replace(prob, P=rows_ref["P_new"]), dense_noise=False)
        assert res.status == want["status"] == 0 and np.array_equal(res.accepted, want["accepted"])
        assert 0 < int(res.accepted.sum()) < prob.F and res.accepted.shape == (prob.F,)
        e = fp.metrics(res.dx, res.P_new, want, rows_ref["P_new"])
        print("ROWS rows_then_camera " + " ".join(f"{x:.2e}" for x in e))
        assert max(e) < TOL, e
        assert code(eng.rows_gate) == -5                                 # the last run is a camera run
        # the other order: the camera update committed, then rows on its P+
        eng.set_state(prob)
        eng.set_features(prob)
        eng.run()
        first = eng.result()
        assert first.status == 0 and np.array_equal(first.accepted, cam_ref["accepted"])
        assert eng.commit_covariance() == 0
        P_cam = np.array(cam_ref["P_new"])
        S = rr.pad(H, P_cam.shape[0]) @ P_cam @ rr.pad(H, P_cam.shape[0]).T + R
        r2 = np.linalg.cholesky((S + S.T) / 2) @ np.array([0.3, -1.1, 0.6])
        res2 = eng.update_rows(H, r2, R)
        check("camera_then_rows", res2, rr.update(P_cam, H, r2, R), P_cam)
        # ... and the batch is still there
        eng.run()
        assert eng.result().accepted.shape == (prob.F,)
