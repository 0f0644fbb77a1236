"""A K5 plan miss clears nothing and rebuilds only what changed.

Band plans in k_sweep form keep the root block and the zero words at the head of the R workspace, cleared once per
(allocation, dc); the leaves' and the merges' blocks behind them move with the leaf counts and are never cleared again.  With
MSCKF_DEBUG_POISON=1 every new workspace and every skipped clear is filled with NaN, so an entry that is read without having
been written in the same run shows in dx / P+.  Every comparison is bitwise, against a fresh engine (freshly cleared
workspace, no poison) given the same batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("MSCKF_DEBUG_POISON", "MSCKF_PLAN_MEMO", "MSCKF_DEBUG_FAKE_TIMEOUT", "MSCKF_ROOT_STREAM", "MSCKF_LEAF_STREAM", "MSCKF_GAIN_STREAM")


def _engine(monkeypatch, poison=False, memo=True, **kw):
    """The switches are read by msckf_create: set for this engine only."""
    from msckf_amd.api import UpdateEngine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if poison:
        monkeypatch.setenv("MSCKF_DEBUG_POISON", "1")
    if not memo:
        monkeypatch.setenv("MSCKF_PLAN_MEMO", "0")
    kw = {**dict(max_clones=30, max_features=2048, max_track=31), **kw}
    eng = UpdateEngine(**kw)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return eng


def take(prob, idx):
    """The batch of `prob`'s tracks idx, in that order, on the same state."""
    from msckf_amd import synth
    idx = np.asarray(idx)
    M = np.diff(prob.view_ptr)
    vp = np.zeros(len(idx) + 1, dtype=np.int32)
    vp[1:] = np.cumsum(M[idx])
    views = np.concatenate([np.arange(prob.view_ptr[f], prob.view_ptr[f + 1]) for f in idx])
    q = synth.UpdateProblem(**{**prob.__dict__})
    q.view_ptr = vp
    q.obs_uv = prob.obs_uv[views].copy(); q.obs_slot = prob.obs_slot[views].copy()
    q.idp_base = prob.idp_base[idx].copy(); q.idp_m = prob.idp_m[idx].copy(); q.idp_rho = prob.idp_rho[idx].copy()
    return q


def first_slots(prob):
    return np.array([prob.obs_slot[prob.view_ptr[f]:prob.view_ptr[f + 1]].min() for f in range(prob.F)])


def group_hist(prob, N):
    return np.bincount(first_slots(prob), minlength=N)


def skewed_batch(N, F, M, k, peak, share, single=None, **kw):
    """F tracks out of a seeded pool of 10 F: `share` of them start at slot `peak` (that group's leaf count moves with it), the
    others are spread evenly; `single`: a group (first slot) cut down to three tracks, one leaf whatever the shape."""
    from msckf_amd import synth
    pool = synth.make_problem(N, 10 * F, M, seed=900 + k, **kw)
    fs = first_slots(pool)
    rng = np.random.default_rng(7000 + k)
    groups = [g for g in range(N - M + 1)]
    n_peak = int(round(share * F))
    want = {g: 0 for g in groups}
    want[peak] = n_peak
    rest = [g for g in groups if g != peak]
    if single is not None:
        want[single] = 3
        rest = [g for g in rest if g != single]
    left = F - sum(want.values())
    for i, g in enumerate(rest):
        want[g] += left // len(rest) + (1 if i < left % len(rest) else 0)
    idx = []
    for g in groups:
        have = np.flatnonzero(fs == g)
        assert len(have) >= want[g], (g, len(have), want[g])
        idx.extend(rng.choice(have, size=want[g], replace=False))
    idx = rng.permutation(np.array(idx))
    assert len(idx) == F
    return take(pool, idx)


# (N, F, M) -> per batch (peak group, its share of the tracks, extra).  Consecutive batches (the rotation's wrap-around included)
# differ in the peak group's leaf count: a leaf takes 40 tracks of 5 views, 16 of 8 or 10 (build_plan_band).
SHAPES = {
    (10, 50, 5): [(0, 0.90, {}), (3, 0.20, {}), (5, 0.84, dict(outlier_fraction=0.1, outlier_px=500.0)), (1, 0.10, dict(single=4)),
                  (2, 0.86, dict(sigma=0.01, pixel_noise=80.0)), (4, 0.16, {})],
    (20, 500, 8): [(0, 0.40, {}), (6, 0.08, {}), (12, 0.30, dict(outlier_fraction=0.1, outlier_px=500.0)), (3, 0.10, dict(single=9)),
                   (7, 0.36, dict(sigma=0.01, pixel_noise=80.0)), (10, 0.12, {})],
    (30, 400, 10): [(0, 0.30, {}), (9, 0.06, {}), (20, 0.26, dict(outlier_fraction=0.1, outlier_px=500.0)), (5, 0.10, dict(single=13)),
                    (14, 0.28, dict(sigma=0.01, pixel_noise=80.0)), (17, 0.12, {})],
}
_cache = {}


def batches(shape):
    if shape not in _cache:
        N, F, M = shape
        out = []
        for k, (peak, share, extra) in enumerate(SHAPES[shape]):
            extra = dict(extra)
            single = extra.pop("single", None)
            out.append(skewed_batch(N, F, M, 31 * N + k, peak, share, single=single, **extra))
        _cache[shape] = out
    return _cache[shape]


def fresh(monkeypatch, prob, **kw):
    with _engine(monkeypatch, **kw) as eng:
        return eng.update_problem(prob)


def same(a, b):
    return (a.status == b.status and np.array_equal(a.dx, b.dx) and np.array_equal(a.P_new, b.P_new) and
            np.array_equal(a.accepted, b.accepted))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_same_class_moving_leaves(monkeypatch, shape):
    N, F, M = shape
    probs = batches(shape)
    refs = [fresh(monkeypatch, p) for p in probs]
    # what the batches are there for
    assert refs[2].accepted.sum() < F and refs[2].status == 0                  # gross outliers, some rejected
    assert group_hist(probs[3], N)[SHAPES[shape][3][2]["single"]] == 3         # a group of one leaf
    assert refs[4].accepted.sum() == 0 and refs[4].status == 1                 # nothing accepted: no-op
    with _engine(monkeypatch, poison=True) as eng:
        last_leaves = None
        for i in range(2 * len(probs)):
            k = i % len(probs)
            r = eng.update_problem(probs[k])
            assert same(r, refs[k]), (shape, i)
            assert r.stats["n_leaves"] == refs[k].stats["n_leaves"] and r.stats["stacked_rows"] == refs[k].stats["stacked_rows"]
            assert r.stats["n_leaves"] != last_leaves, (shape, i)             # the leaf count moved: a plan miss, blocks elsewhere
            last_leaves = r.stats["n_leaves"]


def _select_update(eng, prob, seed):
    from msckf_amd import synth
    tracks = synth.make_tracks(prob, seed, lost_fraction=0.5)
    params = synth.SelectParams(use_parallax=False)
    eng.load(prob)
    eng.set_tracks(tracks)
    eng.run_select(params, prob.K)
    eng.replan()
    eng.run()
    return eng.result()


@pytest.mark.parametrize("plan", ["auto", "tree"])
def test_key_changes(monkeypatch, plan):
    from msckf_amd import synth
    band = synth.make_problem(30, 300, 10, seed=41)
    band2 = synth.make_problem(30, 340, 10, seed=42, outlier_fraction=0.1, outlier_px=400.0)
    split = synth.make_problem(30, 200, 30, seed=43, variable_tracks=True, min_track=2)
    small = synth.make_problem(12, 100, 5, seed=44)
    steps = [("update", band), ("update", split), ("update", band), ("update", small), ("update", band2), ("select", band),
             ("update", band2), ("update", band)]
    with _engine(monkeypatch, poison=True, plan=plan) as eng:
        for i, (kind, prob) in enumerate(steps):
            if kind == "update":
                got = eng.update_problem(prob)
                with _engine(monkeypatch, plan=plan) as ref_eng:
                    ref = ref_eng.update_problem(prob)
            else:
                got = _select_update(eng, prob, 51)
                with _engine(monkeypatch, plan=plan) as ref_eng:
                    ref = _select_update(ref_eng, prob, 51)
                assert 0 < ref.stats["n_features"] < prob.F                    # the selection dropped tracks: the re-plan is smaller
            assert ref.status == 0 and same(got, ref), (plan, i, kind)
            if prob is split and plan == "auto":
                assert eng.debug_split()["long_tracks"] > 0


def test_resident_calls(monkeypatch):
    probs = batches((20, 500, 8))
    refs = [fresh(monkeypatch, p) for p in probs]
    with _engine(monkeypatch, poison=True) as eng:
        for i in range(2 * len(probs)):
            k = i % len(probs)
            eng.load(probs[k])
            eng.run()
            assert same(eng.result(), refs[k]), i


@pytest.mark.parametrize("N,F", [(12, 300), (30, 600)])
def test_planner_memo(monkeypatch, N, F):
    """Ragged batches: the group shapes differ from call to call, so the memo is asked for tables it has, tables it has not and
    tables it had a few calls ago.  With and without it every result and every stats field is the same, call by call."""
    from msckf_amd import synth
    probs = [synth.make_problem(N, F - 20 * k, 10, seed=60 + k, variable_tracks=True, min_track=2) for k in range(4)]
    timing = ("us_total", "us_feature", "us_qr", "us_gain", "us_host_prep", "us_h2d", "us_d2h")
    with _engine(monkeypatch, poison=True) as a, _engine(monkeypatch, poison=True, memo=False) as b:
        for i in range(3 * len(probs)):
            p = probs[(i * 3) % len(probs)] if i % 2 else probs[i % len(probs)]
            ra, rb = a.update_problem(p), b.update_problem(p)
            assert same(ra, rb) and ra.status == 0, (N, i)
            assert {k: v for k, v in ra.stats.items() if k not in timing} == {k: v for k, v in rb.stats.items() if k not in timing}, (N, i)


def test_retry_path():
    """MSCKF_DEBUG_FAKE_TIMEOUT=1: the first streamed update of every context reads as timed out and is rerun on plain launches,
    where the context stays.  The switch is read once per process: a child process."""
    code = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import msckf_amd
from msckf_amd.api import UpdateEngine
from test_gpu_plan_miss import batches, same
probs = batches((20, 500, 8))[:4]
os.environ["MSCKF_DEBUG_POISON"] = "1"
eng = UpdateEngine(max_clones=30, max_features=2048, max_track=31)
del os.environ["MSCKF_DEBUG_POISON"]
ok = True
for i in range(6):
    p = probs[i %% 4]
    got = eng.update_problem(p)
    with UpdateEngine(max_clones=30, max_features=2048, max_track=31) as ref_eng:
        ref = ref_eng.update_problem(p)                     # (its first update: retried as well)
    good = ref.status == 0 and same(got, ref)
    print("call", i, "leaves", got.stats["n_leaves"], "k5 launches", got.stats["k5_launches"], "same", good, flush=True)
    ok = ok and good and got.stats["k5_launches"] == ref.stats["k5_launches"] >= 3      # leaves, merges and root as launches of their own
eng.close()
print("RETRY_OK" if ok else "RETRY_BAD")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["MSCKF_DEBUG_FAKE_TIMEOUT"] = "1"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert "RETRY_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
