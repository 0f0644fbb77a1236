"""`dtype = f32` on filter-shaped priors (tests/filter_prior.py), held to its fp32 rounding budget in covariance units.

tests/test_gpu_f32.py holds the mode to a per-case budget on recipe-A priors and in `rel_err` only; on a prior a filter made,
`rel_err` over the whole of dx or P+ cannot see a block left at the prior's value.  Here every update is
held in the five measures of `filter_prior.metrics` -- rel_err on dx and P+, scaled_dx, scaled_P, update_term -- to
`f32_model.bound_measures` of the model's budget over 16 null-space bases:

  1  the streamed update, one-shot and load / run: families forms, stream, plan; long_31 / 53 / 64 with fp64 products (split long
     tracks); engines of 53 and of 82 clones.  long_65 -- long tracks past the split's limit, unsplit to the
     merge tree -- reports fp32 products, but its root is as wide as the window, the streamed K6-K7 does not fit
     (gstream_ok) and the CHAIN runs: P+ arrives as widened floats, and the case is held to the chain's budget
  2  three updates with commit_covariance() in between on filter_prior(12) and filter_prior(30), against `budget_sequence`
  3  the chain (`launch_gain`: the Joseph products on k_gemm_f32), each environment in a child process of its own, against
     `f32_model.chain_budget_measures`: MSCKF_GAIN_STREAM=0 on family forced and on the recipe-A problems of
     test_gpu_wide_windows.FORCED at the same N; no switch at chain_83 and chain_107; MSCKF_DEBUG_FAKE_TIMEOUT=1 at N = 60 and 82,
     both updates of a fresh engine
  (4  test_gpu_f32.test_golden_f32[edge_gauge_prior] takes its bounds on P+, scaled_dx and scaled_P from the same model; its
      update_term is in OUTSIDE below.)

Every check prints `F32COV <case> <measure> e/b ...` (`-s`); the largest per family are in DESIGN.md section 5.  The cases were
conditioned on the CPU first (tests/test_f32_filter_prior.py: the model is the oracle without rounding, the budget is stable, the
caps do not bind, diag(P+) > 0); a case that missed a condition is in OUTSIDE below and runs on the flat pair alone.

On the flat pair only: chain_187, chain_221 and the two `few` cases (d = 1137 and 1341).  One sample of the chain model at
d = 1341 took 1.6 s on two CPU threads (the QR of the stack, the fp64 solve and the three products), sixteen 25 s, and two sets
for the CPU conditions of four such cases over 3 minutes -- against 0.1 - 6.4 s for two sets of any case up to d = 657.

Which path ran is read off the result: `k_symmetrize_f32` stores P+ as widened floats, the streamed update keeps it in fp64."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import f32_model as fm
import filter_prior as fp
from conftest import ROOT

pytestmark = pytest.mark.gpu

MEASURES = ("e_dx", "e_P", "s_dx", "s_P", "u_P")

# ---- the cases ------------------------------------------------------------------------------------------------------------------

# name -> what the budget assumes: True the streamed update with fp32 products, False with fp64 products (split long tracks),
# "chain" the chain behind a merge tree as wide as the window
STREAMED = {n: True for n, c in fp.CASES.items() if c.family in ("forms", "stream", "plan")}
STREAMED.update({"long_31": False, "long_53": False, "long_64": False, "long_65": "chain"})
SEQ_N = (12, 30)
SEQ_SEED = 22700                       # + N + 100 * step: family f's recipe (tests/test_gpu_f32.py) on a filter prior
RETRY_N = (60, 82)
RETRY_SEED = (22800, 22850)            # + N: the two batches of one context
FORCED_A_N = (10, 11, 21, 22, 31, 32, 53, 54, 82)       # test_gpu_wide_windows.FORCED's f32 problems at family forced's widths
CHAIN_FLAT = ("chain_187", "chain_221", "chain_221_F1", "chain_221_F2")

# A case that missed a condition of tests/test_f32_filter_prior.py: name -> (measure, value, condition).  It runs on the flat
# pair only (at most two may stand here).
#   chain_83          rel_err on dx 1.87e-6 over samples 1 - 16, 3.98e-6 over 17 - 32: not within a factor 2 (dx is fp64 on the
#                     chain: this is the fp32 stack alone, in a basis-dependent tail)
#   edge_gauge_prior  update_term 5.7e-3: MARGIN * b = 2.3e-2 is past the 1e-4 cap -- the 100 m^2 of gauge variance the fp32 stack
#                     cannot keep out of the update (tests/test_gpu_f32.py).  Its flat pair is the fixture's 0.2 / 1e-2; the test
#                     still takes P+, scaled_dx and scaled_P from the model, whose caps hold, and update_term from MARGIN * b alone
OUTSIDE = {"chain_83": ("e_dx", (1.87e-6, 3.98e-6), "stable"), "edge_gauge_prior": ("u_P", 5.7e-3, "cap")}


def _family(*families):
    return [n for n, c in fp.CASES.items() if c.family in families]


@functools.lru_cache(maxsize=None)
def chain_problem(spec):
    """(prob, oracle result) of ("fp", name): a case of filter_prior.CASES; ("A", N): test_gpu_wide_windows.FORCED's problem;
    ("retry", N, i): batch i of the retried context, T full, on filter_prior(N).  Computed once: leave both unchanged."""
    from oracle import msckf_oracle as oracle
    import test_gpu_wide_windows as ww
    if spec[0] == "fp":
        return fp.problem(spec[1])
    if spec[0] == "A":
        prob = ww.problem("full", spec[1], 4800 + spec[1])
    else:
        N = spec[1]
        P, cam_R, cam_t, _, _ = fp.filter_prior(N)
        prob = ww.full_problem(N, RETRY_SEED[spec[2]] + N, P=np.array(P), poses=(cam_R, cam_t))
    return prob, oracle.update(prob, dense_noise=False)


FORCED = {n: ("fp", n) for n in _family("forced")}
FORCED.update({f"A_{N}": ("A", N) for N in FORCED_A_N})
WIDE = {n: ("fp", n) for n in ("chain_83", "chain_107") + CHAIN_FLAT}
RETRY = {f"retry_{N}": [("retry", N, 0), ("retry", N, 1)] for N in RETRY_N}


@functools.lru_cache(maxsize=None)
def sequence(N):
    """Three batches on filter_prior(N), each built on the oracle's P+ of the one before."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    P, cam_R, cam_t, _, _ = fp.filter_prior(N)
    probs, refs = [], []
    for step in range(3):
        probs.append(synth.make_problem(N, 120, 8, seed=SEQ_SEED + N + 100 * step, P=np.array(P), poses=(cam_R, cam_t),
                                        variable_tracks=True, outlier_fraction=0.1, outlier_px=300.0))
        refs.append(oracle.update(probs[-1], dense_noise=False))
        P = refs[-1]["P_new"]
    return probs, refs


@functools.lru_cache(maxsize=None)
def streamed_budget(name, products, first=0):
    prob, ref = fp.problem(name)
    return fm.budget_measures(prob, ref, products, first=first)[0]


@functools.lru_cache(maxsize=None)
def chain_budget(spec, first=0):
    prob, ref = chain_problem(spec)
    return fm.chain_budget_measures(prob, ref, first=first)[0]


# ---- the assertion of every test ------------------------------------------------------------------------------------------------

def is_widened_f32(P):
    return bool(np.array_equal(P, P.astype(np.float32).astype(np.float64)))


def hold(what, e, b, flat_only=False):
    """The five measures `e` within `bound_measures(b)` (flat_only: the flat pair on the two rel_err columns); prints the line."""
    if flat_only or b is None:
        print(f"F32COV {what} flat pair only " + " ".join(f"{m} {x:.2e}" for m, x in zip(MEASURES, e)))
        assert e[0] <= fm.FLAT_DX and e[1] <= fm.FLAT_P, (what, e)
        return
    print(f"F32COV {what} " + " ".join(f"{m} {x:.2e}/{y:.2e}={x / y:.2f}" for m, x, y in zip(MEASURES, e, b)))
    t = fm.bound_measures(b)
    assert all(x <= y for x, y in zip(e, t)), (what, dict(zip(MEASURES, zip(e, t))))


def hold_result(what, eng, res, prob, ref, products, budget=None):
    """Status and mask are the oracle's, P+ is bit-symmetric with a positive diagonal and came from the K6-K7 the budget assumes,
    the product mode is the planner's, the five measures are within the bound."""
    assert res.status == ref["status"]
    assert np.array_equal(res.accepted, ref["accepted"])
    if res.status != 0:                                      # the no-op contract
        assert np.array_equal(res.P_new, prob.P) and not res.dx.any()
        return
    assert np.array_equal(res.P_new, res.P_new.T)
    assert (np.diag(res.P_new) > 0).all()
    assert is_widened_f32(res.P_new) == (products == "chain")
    s = eng.debug_split()
    fp64_products = s["long_tracks"] > 0 and s["band_plan"] == 1
    assert bool(products) == (not fp64_products), s
    name = what.split(" ")[0]
    if budget is None and name not in OUTSIDE:
        budget = chain_budget(("fp", name)) if products == "chain" else streamed_budget(name, products)
    hold(f"{what} products={products}", fp.metrics(res.dx, res.P_new, ref, prob.P), budget, flat_only=name in OUTSIDE)


# ---- 1. the streamed update -----------------------------------------------------------------------------------------------------

def _engine(N):
    from msckf_amd.api import UpdateEngine
    return UpdateEngine(max_clones=N, max_features=512, max_track=31, dtype="f32")


@pytest.fixture(scope="module")
def eng53():
    e = _engine(53)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng82():
    e = _engine(82)
    yield e
    e.close()


def _streamed(eng, name):
    prob, ref = fp.problem(name)
    hold_result(f"{name} one-shot", eng, eng.update_problem(prob), prob, ref, STREAMED[name])
    eng.load(prob)
    eng.run()
    hold_result(f"{name} load/run", eng, eng.result(), prob, ref, STREAMED[name])
    return ref


@pytest.mark.parametrize("name", [n for n in STREAMED if fp.CASES[n].N <= 53])
def test_streamed_update_in_covariance_units(eng53, name):
    """forms (every solve dispatch below 54 clones; forms_1 is the no-op), plan (the K5 plan's boundaries), long_31 and long_53
    (split long tracks: fp64 products)."""
    ref = _streamed(eng53, name)
    assert (ref["status"] != 0) == (name in fp.NO_ROWS)
    if fp.CASES[name].family == "long":
        assert eng53.debug_split()["long_tracks"] > 0


@pytest.mark.parametrize("name", [n for n in STREAMED if fp.CASES[n].N > 53])
def test_streamed_update_in_covariance_units_wide(eng82, name):
    """stream (54 - 82 clones), long_64 (the widest split) and long_65 (unsplit, to the merge tree and the chain)."""
    ref = _streamed(eng82, name)
    assert ref["status"] == 0
    if fp.CASES[name].family == "long":
        assert (eng82.debug_split()["long_tracks"] > 0) == (fp.CASES[name].N <= 64)


# ---- 2. the committed sequence --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", SEQ_N)
def test_committed_sequence_in_covariance_units(eng53, N):
    """Three updates with commit_covariance() in between: the engine starts step k from its own fp32-rounded P+, the model carries
    its own through the same steps, and both are measured against the oracle, the scaled measures on the oracle's prior."""
    probs, refs = sequence(N)
    budgets, _ = fm.budget_sequence(probs, refs, True)
    eng53.load(probs[0])
    for k, (prob, ref) in enumerate(zip(probs, refs)):
        if k:
            assert eng53.commit_covariance() == 0
            eng53.set_features(prob)
        eng53.run()
        assert ref["status"] == 0
        hold_result(f"seq_{N} step{k + 1}", eng53, eng53.result(), prob, ref, True, budget=budgets[k])


# ---- 3. the chain ---------------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import msckf_amd
from msckf_amd.api import UpdateEngine
import filter_prior as fp
import test_gpu_f32_filter_prior as m
cases = json.loads(%(cases)r)
shared = None
out = {}
for name, specs in cases.items():
    if %(fresh)d:
        e = UpdateEngine(max_clones=specs[0][1], max_features=512, max_track=31, dtype="f32")
    else:
        e = shared = shared or UpdateEngine(max_clones=%(max_n)d, max_features=512, max_track=31, dtype="f32")
    out[name] = []
    for spec in specs:
        prob, ref = m.chain_problem(tuple(spec))
        r = e.update_problem(prob)
        out[name].append(dict(status=int(r.status), ref_status=int(ref["status"]), acc=bool(np.array_equal(r.accepted, ref["accepted"])),
                              sym=bool(np.array_equal(r.P_new, r.P_new.T)), diag=float(np.diag(r.P_new).min()),
                              widened_f32=m.is_widened_f32(r.P_new), err=e._lib.msckf_last_error(e._h).decode(),
                              metrics=[float(x) for x in fp.metrics(r.dx, r.P_new, ref, prob.P)]))
    if %(fresh)d:
        e.close()
if shared is not None:
    shared.close()
print("RESULT " + json.dumps(out))
"""


def _run(env_extra, cases, max_n, fresh=False):
    code = CHILD % dict(root=ROOT, cases=json.dumps(cases), max_n=max_n, fresh=int(fresh))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env_extra))
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1][len("RESULT "):])


def _hold_chain(what, r, spec, flat_only=False):
    assert r["status"] == r["ref_status"] == 0 and r["acc"], r
    assert r["sym"] and r["diag"] > 0, r
    assert r["widened_f32"], r                               # k_symmetrize_f32's store: the chain ran
    flat_only = flat_only or what in OUTSIDE
    hold(what, r["metrics"], None if flat_only else chain_budget(spec), flat_only=flat_only)


@pytest.fixture(scope="module")
def forced():
    return _run({"MSCKF_GAIN_STREAM": "0"}, {n: [list(s)] for n, s in FORCED.items()}, 82)


@pytest.mark.parametrize("name", list(FORCED))
def test_chain_forced_in_covariance_units(forced, name):
    """MSCKF_GAIN_STREAM=0: every solve dispatch of the chain below 83 clones, T full, on the filter prior (forced_N) and on the
    recipe-A prior (A_N)."""
    _hold_chain(name, forced[name][0], FORCED[name])


@pytest.fixture(scope="module")
def wide():
    return _run({}, {n: [list(s)] for n, s in WIDE.items()}, fp.MAX_N)


@pytest.mark.parametrize("name", list(WIDE))
def test_chain_past_82_clones_in_covariance_units(wide, name):
    """The chain as the only K6-K7: chain_83 and chain_107 against the model; d = 1137 - 1341 on the flat pair (the header)."""
    _hold_chain(name, wide[name][0], WIDE[name], flat_only=name in CHAIN_FLAT)


@pytest.fixture(scope="module")
def retried():
    return _run({"MSCKF_DEBUG_FAKE_TIMEOUT": "1"}, {n: [list(s) for s in specs] for n, specs in RETRY.items()}, 0, fresh=True)


@pytest.mark.parametrize("name", list(RETRY))
def test_timeout_retry_in_covariance_units(retried, name):
    """The first update of a fresh f32 context ran the streamed K6-K7, read as timed out and was rerun on the chain; the second
    batch of the same context stays on the chain.  Both are the chain's P+ (widened floats) and are held to the chain's budget."""
    first, second = retried[name]
    assert first["err"] == "k_gain_stream timed out once: this context now runs its sweeps and K6-K7 as separate launches"
    _hold_chain(f"{name} first", first, RETRY[name][0])
    _hold_chain(f"{name} second", second, RETRY[name][1])
