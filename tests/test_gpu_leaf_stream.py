"""The band plan's K5-K7 in one launch (k_leaf_root_gain): the leaves publish their rows as they become final, the merge nodes
fold them as they arrive and stream to the root, the root to the strips of K6-K7.  Every shape below must run that launch
(stats k5_launches == 1), match the oracle, match the two-launch path (MSCKF_LEAF_STREAM=0: the leaves as a launch of their own)
to 1e-12 and give the same bits on 50 repeated calls.  A fake timeout of the fused launch is retried on plain launches, and a
failed gain comes back as MSCKF_ERR_NOT_SPD with the prior untouched.  The environment switches are read once per process:
each setting runs in a child process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# name: (engine (max_clones, max_features, max_track), make_problem arguments)
SHAPES = {
    "headline": ((30, 2048, 10), dict(N=30, F=2000, M=10, seed=11)),
    "cfg1": ((20, 512, 8), dict(N=20, F=500, M=8, seed=12)),
    "ragged": ((30, 1024, 10), dict(N=30, F=1000, M=10, seed=13, variable_tracks=True, min_track=2)),
    "outliers": ((30, 2048, 10), dict(N=30, F=2000, M=10, seed=14, outlier_fraction=0.1, outlier_px=500.0)),
    "single_leaf_groups": ((30, 512, 10), dict(N=30, F=300, M=10, seed=15)),
    "n10": ((10, 512, 6), dict(N=10, F=400, M=6, seed=16)),
}
REPEATS = 50

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import msckf_amd
from msckf_amd import synth
from msckf_amd.api import UpdateEngine
from oracle import msckf_oracle as oracle
from conftest import rel_err
shapes = json.loads(%(shapes)r)
out = {}
for name, (eng_args, kw) in shapes.items():
    prob = synth.make_problem(kw.pop("N"), kw.pop("F"), kw.pop("M"), **kw)
    ref = oracle.update(prob, dense_noise=False)
    with UpdateEngine(max_clones=eng_args[0], max_features=eng_args[1], max_track=eng_args[2]) as e:
        r = e.update_problem(prob)
        same = True
        for _ in range(%(repeats)d - 1):
            q = e.update_problem(prob)
            same = same and np.array_equal(q.dx, r.dx) and np.array_equal(q.P_new, r.P_new)
    np.save(%(tmp)r + "/" + name + "_dx.npy", r.dx)
    np.save(%(tmp)r + "/" + name + "_P.npy", r.P_new)
    out[name] = dict(status=int(r.status), k5=int(r.stats.get("k5_launches", -1)), same=bool(same),
                     acc=bool(np.array_equal(r.accepted, ref["accepted"])), ref_status=int(ref["status"]),
                     e_dx=float(rel_err(r.dx, ref["dx"])), e_P=float(rel_err(r.P_new, ref["P_new"])))
print("RESULT " + json.dumps(out))
"""


def _run(tmp, env_extra, shapes=SHAPES, repeats=REPEATS):
    os.makedirs(tmp, exist_ok=True)
    code = CHILD % dict(root=ROOT, shapes=json.dumps(shapes), repeats=repeats, tmp=str(tmp))
    env = dict(os.environ, **env_extra)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1][len("RESULT "):])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("leaf_stream")
    fused = _run(base / "fused", {})
    plain = _run(base / "plain", {"MSCKF_LEAF_STREAM": "0"}, repeats=1)
    return base, fused, plain


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_launch_matches_oracle_and_two_launches(runs, name):
    base, fused, plain = runs
    f, p = fused[name], plain[name]
    assert f["k5"] == 1, f                      # leaves, merge level, root and K6-K7: one launch
    assert p["k5"] == 2, p                      # the A/B switch: the leaves in a launch of their own
    assert f["status"] == f["ref_status"] == 0 and f["acc"], f
    assert f["e_dx"] < 1e-8 and f["e_P"] < 1e-8, f
    assert f["same"], "repeated calls on the fused launch differ"
    for q in ("dx", "P"):
        a = np.load(base / "fused" / f"{name}_{q}.npy")
        b = np.load(base / "plain" / f"{name}_{q}.npy")
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b), (name, q)


def test_fused_launch_fake_timeout_is_retried(tmp_path):
    """MSCKF_DEBUG_FAKE_TIMEOUT=1: the first update of the context reads as timed out; the retry on plain launches returns the
    right result, and the context stays on those."""
    shapes = {"headline": SHAPES["headline"]}
    r = _run(tmp_path, {"MSCKF_DEBUG_FAKE_TIMEOUT": "1"}, shapes=shapes, repeats=2)["headline"]
    assert r["status"] == 0 and r["acc"] and r["e_dx"] < 1e-8 and r["e_P"] < 1e-8, r
    assert r["k5"] >= 3, r                      # (the retried call's launches: leaves, merge level, root)
    assert r["same"], r


FAIL_CHILD = r"""
import ctypes as C
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import msckf_amd
import failing_batches as fb
from msckf_amd import _ffi
from msckf_amd.api import UpdateEngine, chi2_table
prob = fb.spd_p_problem()
with UpdateEngine(max_clones=30, max_features=512, max_track=10) as e:
    # (msckf_update as UpdateEngine.update_problem calls it, without turning the code into an exception: the stats are wanted too)
    a = e._pack(prob)
    chi = _ffi.f64(chi2_table())
    dx = np.full(prob.d, np.nan)
    P_out = np.full((prob.d, prob.d), np.nan)
    acc = np.zeros(max(prob.F, 1), dtype=np.uint8)
    st = _ffi.Stats()
    rc = e._lib.msckf_update(
        e._h, prob.N, _ffi.dptr(a["P"]), _ffi.dptr(a["cam_R"]), _ffi.dptr(a["cam_t"]), _ffi.dptr(a["cam_R0"]),
        _ffi.dptr(a["cam_t0"]), _ffi.dptr(a["g"]), _ffi.dptr(a["Kinv"]), float(prob.sigma), prob.F,
        _ffi.iptr(a["view_ptr"]), _ffi.dptr(a["obs_uv"]), _ffi.iptr(a["obs_slot"]), _ffi.dptr(a["idp_base"]),
        _ffi.dptr(a["idp_m"]), _ffi.dptr(a["idp_rho"]), _ffi.dptr(chi), int(chi.size),
        _ffi.dptr(dx), _ffi.dptr(P_out), _ffi.uptr(acc), C.byref(st))
    print("RESULT", int(rc), int(st.as_dict().get("k5_launches", -1)), bool(np.all(dx == 0)),
          bool(np.array_equal(P_out, prob.P)), int(_ffi.ERR_NOT_SPD))
"""


def test_fused_launch_reports_a_failed_gain():
    """A batch whose gates all pass but whose joint innovation covariance is indefinite (failing_batches.spd_p_problem, short
    tracks only: the fused launch's form) comes back as MSCKF_ERR_NOT_SPD, dx = 0, P_out the prior."""
    out = subprocess.run([sys.executable, "-c", FAIL_CHILD % dict(root=ROOT)], capture_output=True, text=True, timeout=300)
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert lines, out.stdout[-2000:] + out.stderr[-3000:]
    _, status, k5, dx0, prior, not_spd = lines[-1]
    assert int(status) == int(not_spd), lines[-1]
    assert dx0 == "True" and prior == "True", lines[-1]
    assert int(k5) == 1, lines[-1]
