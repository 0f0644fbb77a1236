"""Windows wider than 53 clones, up to the widest msckf_create accepts (N = 221: k_propagate's LDS tile), against the oracle.

  54 - 82   the streamed K6-K7 (k_gain_stream / k_root_gain*): strip counts 22 - 32 of GS_MAX_NS, the band ring, split long tracks;
  83 - 221  round 3's K6-K7 chain (launch_gain: k_chol<512> on its global-memory branch past dc = 198, k_solve<NREG> up to
            NREG = 21), the K5 plans wider than FOLD_RLDS_MAX_W, long tracks that are not split;
  forced    MSCKF_GAIN_STREAM=0 at every solve dispatch of the chain, both dtypes;
  retry     a timed-out streamed update is rerun on the chain (MSCKF_DEBUG_FAKE_TIMEOUT=1), and the context stays there;
  capacity  max_clones = 221 / 222, propagate / augment / remove and an update on the resident P at N = 221.
Until the fixes that came with these tests the chain solved only the first 320 columns of K for dc > 320 (N >= 54), and the
merge tree's HBM fold kept only the first 320 columns of a node: dx and P+ far off with status 0.  The environment switches
are read once per process: each setting runs in a child process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-8
TOL32_DX, TOL32_P = 1e-4, 1e-5           # dtype = f32 (tests/test_gpu_f32.py)
MAX_N = 221                              # 15 (15 + 6 N) + 225 doubles of k_propagate's LDS tile <= 159 KiB


def short_problem(N, seed, F=90, **state):
    """test_every_window_size's batch: short ragged tracks (at most 10 views), outliers on both sides of the gate.
    `state`: P= and poses= of synth.make_problem, for a prior other than recipe A (tests/filter_prior.py)."""
    from msckf_amd import synth
    M = max(1, min(N, 2 + N % 9))
    return synth.make_problem(N, F, M, seed=seed, variable_tracks=M > 2, outlier_fraction=0.15, outlier_px=300.0, **state)


def long_problem(N, seed, F=90, M=31, min_track=2, **state):
    from msckf_amd import synth
    return synth.make_problem(N, F, M, seed=seed, variable_tracks=True, min_track=min_track, outlier_fraction=0.15,
                              outlier_px=300.0, **state)


def full_problem(N, seed, **state):
    """Short ragged tracks (2 - 10 views) and enough of them (F = 2 N) that the stack has more rows than the window has columns:
    T is full, so every column of K and of the solve is exercised."""
    from msckf_amd import synth
    return synth.make_problem(N, max(90, 2 * N), 10, seed=seed, variable_tracks=True, outlier_fraction=0.15, outlier_px=300.0,
                              **state)


def problem(kind, N, seed):
    if kind == "short":
        return short_problem(N, seed)
    if kind == "full":
        return full_problem(N, seed)
    return long_problem(N, seed, F=60, min_track=11)


def check(res, ref, prob, tol_dx=TOL, tol_p=TOL, populated=True):
    assert res.status == ref["status"]
    assert np.array_equal(res.accepted, ref["accepted"])
    if populated:
        assert 0 < int(ref["accepted"].sum()) < prob.F                # both sides of the gate are populated
    e_dx, e_P = rel_err(res.dx, ref["dx"]), rel_err(res.P_new, ref["P_new"])
    assert e_dx < tol_dx and e_P < tol_p, (e_dx, e_P)
    if res.status == 0:
        assert np.array_equal(res.P_new, res.P_new.T)


@pytest.fixture(scope="module")
def eng():
    from msckf_amd.api import UpdateEngine
    e = UpdateEngine(max_clones=MAX_N, max_features=512, max_track=31)
    yield e
    e.close()


# ---- a. the default path at every strip count of the streamed K6-K7 ------------------------------------------------------------

@pytest.mark.parametrize("N", list(range(54, 83)))
def test_streamed_every_strip_count(eng, N):
    """N = 54 - 82: strip counts 22 - 32 of k_gain_stream / k_root_gain* (ceil(6 N / 16) + 1), the band ring (N > 37)."""
    from oracle import msckf_oracle as oracle
    prob = short_problem(N, 4300 + N, F=4 * N)
    ref = oracle.update(prob, dense_noise=False)
    check(eng.update_problem(prob), ref, prob)


@pytest.mark.parametrize("N", [54, 60, 64, 65, 70, 82])
def test_streamed_long_tracks(eng, N):
    """Tracks of up to 31 views at the widest streamed windows.  Up to N = 64 they are split into narrow blocks + dense
    remainder rows; past it the dense remainder's K6-K7 (gstream_ok_dc: ncb = nb row-block partials in LDS) no longer fits, and
    they go unsplit to the merge tree, whose nodes are wider than FOLD_RLDS_MAX_W (k_fold_g with 391 - 493 columns)."""
    from oracle import msckf_oracle as oracle
    prob = long_problem(N, 4400 + N)
    ref = oracle.update(prob, dense_noise=False)
    res = eng.update_problem(prob)
    assert (eng.debug_split()["long_tracks"] > 0) == (N <= 64)
    check(res, ref, prob)


# ---- b. above 82 clones: the chain is every update ----------------------------------------------------------------------------

WIDE_N = [83, 84, 85, 96, 107, 128, 150, 187, 200, 220, 221]


@pytest.mark.parametrize("N", WIDE_N)
def test_chain_short_tracks(eng, N):
    """dc = 498 - 1326, T full: k_solve<NREG> from NREG = 8 to 21, k_chol<512> in global memory."""
    from oracle import msckf_oracle as oracle
    prob = full_problem(N, 4500 + N)
    ref = oracle.update(prob, dense_noise=False)
    check(eng.update_problem(prob), ref, prob)


@pytest.mark.parametrize("N", [83, 107, 187, 221])
def test_chain_long_tracks(eng, N):
    """Tracks of 11 - 31 views, which the chain takes without a split: the merge tree's k_fold_g up to dc + 1 = 1327 columns
    (until these tests its widest instance held 320, and the columns past it -- r_n among them -- were dropped)."""
    from oracle import msckf_oracle as oracle
    prob = long_problem(N, 4600 + N, F=60, min_track=11)
    ref = oracle.update(prob, dense_noise=False)
    check(eng.update_problem(prob), ref, prob)


@pytest.mark.parametrize("F", [1, 2])
def test_chain_fewest_features_at_capacity(eng, F):
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(MAX_N, F, 8, seed=4700 + F)
    ref = oracle.update(prob, dense_noise=False)
    check(eng.update_problem(prob), ref, prob, populated=False)


# ---- c. the chain forced at every solve dispatch (MSCKF_GAIN_STREAM=0), both dtypes -------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import msckf_amd
from msckf_amd.api import UpdateEngine
from oracle import msckf_oracle as oracle
from conftest import rel_err
from test_gpu_wide_windows import problem
cases = json.loads(%(cases)r)
shared = {}
out = {}
for name, c in cases.items():
    if c["fresh"]:
        e = UpdateEngine(max_clones=c["N"], max_features=512, max_track=31, dtype=c["dtype"])
    else:
        e = shared.get(c["dtype"]) or shared.setdefault(c["dtype"], UpdateEngine(max_clones=%(max_n)d, max_features=512,
                                                                                  max_track=31, dtype=c["dtype"]))
    out[name] = []
    for seed in c["seeds"]:
        prob = problem(c["kind"], c["N"], seed)
        ref = oracle.update(prob, dense_noise=False)
        r = e.update_problem(prob)
        out[name].append(dict(status=int(r.status), ref_status=int(ref["status"]), acc=bool(np.array_equal(r.accepted, ref["accepted"])),
                              n_acc=int(ref["accepted"].sum()), F=int(prob.F), e_dx=float(rel_err(r.dx, ref["dx"])),
                              e_P=float(rel_err(r.P_new, ref["P_new"])), sym=bool(np.array_equal(r.P_new, r.P_new.T)),
                              err=e._lib.msckf_last_error(e._h).decode()))
    if c["fresh"]:
        e.close()
for e in shared.values():
    e.close()
print("RESULT " + json.dumps(out))
"""


def _run(env_extra, cases):
    code = CHILD % dict(root=ROOT, cases=json.dumps(cases), max_n=MAX_N)
    env = dict(os.environ, **env_extra)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1][len("RESULT "):])


def _check_run(r, tol_dx=TOL, tol_p=TOL):
    assert r["status"] == r["ref_status"] and r["acc"], r
    assert 0 < r["n_acc"] < r["F"], r
    assert r["e_dx"] < tol_dx and r["e_P"] < tol_p, r
    if r["status"] == 0:
        assert r["sym"], r


# k_chol16 + k_solve_lds<1..3> (packed L) | the blocked 2 x 2 gain | k_chol<512> + k_solve<NREG>; full T.  Long tracks: the merge
# tree on either side of k_fold_g's 320 columns.
FORCED_N = [10, 11, 21, 22, 31, 32, 53, 54, 64, 75, 82, 107, 221]
FORCED = {f"{dt}_{N}": dict(N=N, kind="full", dtype=dt, seeds=[4800 + N], fresh=False) for dt in ("f64", "f32") for N in FORCED_N}
FORCED.update({f"{dt}_long_{N}": dict(N=N, kind="long", dtype=dt, seeds=[4850 + N], fresh=False)
               for dt in ("f64", "f32") for N in (53, 54, 82)})


@pytest.fixture(scope="module")
def forced():
    return _run({"MSCKF_GAIN_STREAM": "0"}, FORCED)


@pytest.mark.parametrize("name", list(FORCED))
def test_chain_forced(forced, name):
    tol = (TOL, TOL) if FORCED[name]["dtype"] == "f64" else (TOL32_DX, TOL32_P)
    _check_run(forced[name][0], *tol)


# ---- d. the timeout retry at wide windows ------------------------------------------------------------------------------------

RETRY = {f"retry_{N}": dict(N=N, kind="full", dtype="f64", seeds=[4900 + N, 4950 + N], fresh=True) for N in (60, 82)}


@pytest.fixture(scope="module")
def retried():
    return _run({"MSCKF_DEBUG_FAKE_TIMEOUT": "1"}, RETRY)


@pytest.mark.parametrize("name", list(RETRY))
def test_timeout_retry_on_the_chain(retried, name):
    """The first update ran the streamed K6-K7 (a k_gain_stream launch of its own at these windows), read as timed out and was
    rerun on round 3's chain; the second batch of the same context stays on it.  Both against the oracle."""
    first, second = retried[name]
    assert first["err"] == "k_gain_stream timed out once: this context now runs its sweeps and K6-K7 as separate launches"
    _check_run(first)
    _check_run(second)


# ---- e. the capacity edge and the resident ops at N = 221 ---------------------------------------------------------------------

def test_capacity_edge():
    from msckf_amd import _ffi
    from msckf_amd.api import UpdateEngine
    with UpdateEngine(max_clones=MAX_N, max_features=16, max_track=8) as e:
        assert e.n_clones == 0
    with pytest.raises(_ffi.EngineError) as err:
        UpdateEngine(max_clones=MAX_N + 1, max_features=16, max_track=8)
    assert err.value.code == _ffi.ERR_ARG


def test_resident_ops_and_update_at_capacity(eng):
    """propagate / augment / remove on the resident P at N = 220 - 221 (d = 1341), then one update on it."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    rng = np.random.default_rng(5000)
    prob = synth.make_problem(MAX_N - 1, 10, 4, seed=5001)
    eng.set_prior(prob.P, prob.gravity, prob.K, prob.sigma, prob.cam_R, prob.cam_t)
    P = prob.P
    for _ in range(3):
        Phi = np.eye(15) + 0.01 * rng.standard_normal((15, 15))
        A = rng.standard_normal((15, 15))
        Q = 1e-6 * A @ A.T
        eng.propagate(Phi, Q)
        P = oracle.propagate_covariance(P, Phi, Q)
    got = eng.covariance()
    assert rel_err(got, P) < 1e-13 and np.array_equal(got, got.T)
    J = np.zeros((6, 15))
    J[:3, :3] = rng.standard_normal((3, 3)); J[3:, :3] = rng.standard_normal((3, 3)); J[3:, 12:] = np.eye(3)
    new_R, new_t = prob.cam_R[-1], prob.cam_t[-1] + np.array([0.15, 0.0, 0.0])
    eng.augment(J, new_R, new_t)
    P = oracle.augment_covariance(P, J)
    assert eng.n_clones == MAX_N and rel_err(eng.covariance(), P) < 1e-14
    slots = [MAX_N - 1, 0, 107]
    eng.remove_clones(slots)
    P = oracle.remove_clones_covariance(P, slots)
    got = eng.covariance()
    assert eng.n_clones == MAX_N - 3 and np.array_equal(got, P)         # a pure gather: bit-exact
    eng.augment(J, new_R, new_t + np.array([0.0, 0.1, 0.0]))
    eng.augment(J, new_R, new_t + np.array([0.0, 0.2, 0.0]))
    eng.augment(J, new_R, new_t + np.array([0.0, 0.3, 0.0]))
    for _ in range(3):
        P = oracle.augment_covariance(P, J)
    assert eng.n_clones == MAX_N and rel_err(eng.covariance(), P) < 1e-14
    keep = [i for i in range(MAX_N) if i not in slots]
    cam_R = np.concatenate([prob.cam_R, new_R[None]])[keep]
    cam_t = np.concatenate([prob.cam_t, new_t[None]])[keep]
    cam_R = np.concatenate([cam_R, np.repeat(new_R[None], 3, axis=0)])
    cam_t = np.concatenate([cam_t, new_t + np.array([[0.0, 0.1, 0.0], [0.0, 0.2, 0.0], [0.0, 0.3, 0.0]])])
    eng.set_poses(cam_R, cam_t)
    batch = synth.make_problem(MAX_N, 300, 8, seed=5002, P=eng.covariance(), poses=(cam_R, cam_t), outlier_fraction=0.15,
                               outlier_px=300.0)
    eng.set_features(batch)
    eng.run()
    res = eng.result()
    check(res, oracle.update(batch, dense_noise=False), batch)
