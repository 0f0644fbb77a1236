"""The fp32 budget in covariance units (tests/f32_model.py: `budget_measures`, `chain_update`, `chain_budget_measures`,
`bound_measures`) on the CPU: what every case of tests/test_gpu_f32_filter_prior.py has to meet before it may run on the engine.

  1. Without rounding, `update` and `chain_update` are the oracle: all five measures of `filter_prior.metrics` within the 1e-12
     of `filter_prior.spread`.
  2. The budget is a stable statistic: samples 1 - 16 against samples 17 - 32 within a factor 2, in every measure.
  3. The caps do not bind: MARGIN * budget is below the flat pair on the rel_err columns and below 1e-4 on the scaled ones.
  4. diag(P+) > 0 in every sample of the model.
  5. Family long: the budgets with and without product rounding are at least 2 MARGIN apart on scaled_P.
  6. What the new bound sees that the flat pair does not: defects injected into the model.

A case that misses a condition stands in test_gpu_f32_filter_prior.OUTSIDE with the measure and its value, and this file checks
that it does miss it.  Seen here (`-s` prints, per case, the five budgets of both sample sets): every case passes but chain_83,
whose rel_err on dx -- the fp32 stack alone, dx is fp64 on the chain -- is 1.9e-6 over samples 1 - 16 and 4.0e-6 over 17 - 32,
and edge_gauge_prior, whose update_term budget of 5.7e-3 is past the cap.  The largest MARGIN * budget on a scaled measure
among the others is 3.0e-5 (scaled_P, plan_256, samples 17 - 32)."""
import functools

import numpy as np
import pytest

import f32_model as fm
import filter_prior as fp
import test_gpu_f32_filter_prior as cases
from conftest import load_golden

SPREAD = 1e-12                         # filter_prior.spread's level (tests/test_filter_prior.py)
CAPS = (fm.FLAT_DX, fm.FLAT_P, fm.FLAT_SCALED, fm.FLAT_SCALED, fm.FLAT_SCALED)

# (id, kind, key, products)
ALL = ([(n, "streamed", n, mode) for n, mode in cases.STREAMED.items() if n not in fp.NO_ROWS and mode != "chain"]
       + [(n, "chain", ("fp", n), True) for n, mode in cases.STREAMED.items() if mode == "chain"]
       + [(n, "chain", s, True) for n, s in cases.FORCED.items()]
       + [(n, "chain", s, True) for n, s in cases.WIDE.items() if n not in cases.CHAIN_FLAT]
       + [(f"{n}-{i}", "chain", s, True) for n, specs in cases.RETRY.items() for i, s in enumerate(specs)]
       + [(f"seq_{N}", "seq", N, True) for N in cases.SEQ_N] + [("edge_gauge_prior", "golden", "edge_gauge_prior", True)])


@functools.lru_cache(maxsize=None)
def _sets(kind, key, products):
    """Per step (one but for a sequence): (budget of samples 1 - 16, budget of samples 17 - 32), and min diag(P+) over all of them."""
    dm = []
    if kind == "seq":
        probs, refs = cases.sequence(key)
        a = fm.budget_sequence(probs, refs, products, diag_min=dm)[0]
        b = fm.budget_sequence(probs, refs, products, first=16, diag_min=dm)[0]
        return list(zip(a, b)), min(dm)
    if kind == "chain":
        prob, ref = cases.chain_problem(key)
        blks = fm.blocks(prob, ref)
        a = fm.chain_budget_measures(prob, ref, blks=blks, diag_min=dm)[0]
        b = fm.chain_budget_measures(prob, ref, first=16, blks=blks, diag_min=dm)[0]
    else:
        prob, ref = load_golden(key) if kind == "golden" else fp.problem(key)
        blks = fm.blocks(prob, ref)
        a = fm.budget_measures(prob, ref, products, blks=blks, diag_min=dm)[0]
        b = fm.budget_measures(prob, ref, products, first=16, blks=blks, diag_min=dm)[0]
    return [(a, b)], min(dm)


def _fmt(b):
    return " ".join(f"{m} {x:.2e}" for m, x in zip(cases.MEASURES, b))


def _conditions(name, kind, key, products):
    """The conditions 2 - 4 a case misses: [(condition, measure, value)]."""
    steps, diag = _sets(kind, key, products)
    missed = []
    for a, b in steps:
        for m, x, y, cap in zip(cases.MEASURES, a, b, CAPS):
            if not 0.5 <= x / y <= 2.0:
                missed.append(("stable", m, (x, y)))
            # (edge_gauge_prior keeps the documented 0.2 on dx, tests/test_gpu_f32.py: no bound is taken from that column)
            if fm.MARGIN * max(x, y) >= cap and not (kind == "golden" and m == "e_dx"):
                missed.append(("cap", m, max(x, y)))
    if not diag > 0:
        missed.append(("diag", "P+", diag))
    return missed


@pytest.mark.parametrize("name,kind,key,products", ALL, ids=[c[0] for c in ALL])
def test_the_case_meets_the_conditions(name, kind, key, products):
    """2 - 4.  A case in OUTSIDE misses exactly what the table says; every other case misses nothing."""
    steps, diag = _sets(kind, key, products)
    for k, (a, b) in enumerate(steps):
        print(f"F32COV-CPU {name} step{k + 1} samples 1-16 {_fmt(a)} | samples 17-32 {_fmt(b)} | min diag(P+) {diag:.2e}")
    missed = _conditions(name, kind, key, products)
    if name in cases.OUTSIDE:
        measure, value, condition = cases.OUTSIDE[name]
        assert [(c, m) for c, m, _ in missed] == [(condition, measure)], missed
        assert np.allclose(missed[0][2], value, rtol=0.05), missed
    else:
        assert not missed, missed


def test_the_outside_table_is_short():
    assert len(cases.OUTSIDE) <= 2
    assert all(n in [c[0] for c in ALL] for n in cases.OUTSIDE)


UNROUNDED = [c for c in ALL if c[1] in ("streamed", "chain")]


@pytest.mark.parametrize("name,kind,key,products", UNROUNDED, ids=[c[0] for c in UNROUNDED])
def test_without_rounding_the_models_are_the_oracle(name, kind, key, products):
    """1.  In a random basis of the null spaces: the sequential block form for the streamed cases, the chain for the chain's."""
    prob, ref = cases.chain_problem(key) if kind == "chain" else fp.problem(key)
    stk = fm.stack(prob, ref, np.random.default_rng([7, 0]))
    model = fm.chain_update if kind == "chain" else fm.update
    dx, Pn = model(stk, prob.P, prob.sigma, False, False)
    e = fp.metrics(dx, Pn, ref, prob.P)
    print(f"F32COV-CPU {name} unrounded {_fmt(e)}")
    assert np.array_equal(Pn, Pn.T) and max(e) <= SPREAD, e


@pytest.mark.parametrize("name", ["long_31", "long_53", "long_64"])
def test_long_tracks_separate_the_product_modes_in_scaled_P(name):
    """5.  Family e's rule of tests/test_f32_model.py in the new measure: these batches are held to the budget WITHOUT product
    rounding; were the split rule's switch lost, the engine would land near the budget WITH it, at least 2 MARGIN higher."""
    prob, ref = fp.problem(name)
    with_, without = cases.streamed_budget(name, True), cases.streamed_budget(name, False)
    print(f"F32COV-CPU {name} products fp32 {_fmt(with_)} | fp64 {_fmt(without)} | scaled_P ratio {with_[3] / without[3]:.0f}")
    assert with_[3] >= 2 * fm.MARGIN * without[3]


# ---- 6. what the bound sees that the flat pair does not -------------------------------------------------------------------------

def truncate_to_16_bits(X32):
    """fp32 with the low 7 of its 23 mantissa bits cleared: the precision of a 16-bit mantissa."""
    return (X32.view(np.uint32) & np.uint32(0xFFFFFF80)).view(np.float32)


def _defect(name, operand):
    prob, ref = fp.problem(name)
    stk = fm.stack(prob, ref, np.random.default_rng([99, 0]))
    dx, Pn = fm.chain_update(stk, prob.P, prob.sigma, True, True, operand=operand)
    return fp.metrics(dx, Pn, ref, prob.P), cases.chain_budget(("fp", name))


def _report(what, e, b):
    over = [m for m, x, y in zip(cases.MEASURES, e, b) if x > fm.MARGIN * y]
    flat = e[0] < fm.FLAT_DX and e[1] < fm.FLAT_P
    print(f"F32COV-CPU defect {what}: " + " ".join(f"{m} {x:.2e}={x / y:.0f}b" for m, x, y in zip(cases.MEASURES, e, b))
          + f" | beyond MARGIN * b in {over}; {'PASSES' if flat else 'fails'} the flat pair")
    return over, flat


def test_the_bound_sees_a_truncated_operand_of_a_chain_product():
    """A precision-class defect: T, the second operand of D = sigma^2 K - B2[:, 15:] T^T, with a 16-bit mantissa on forced_31.  dx
    is untouched (fp64).  Seen: rel_err on P+ 1.4e-6 -- a seventh of the flat 1e-5 -- which is 22 budgets, as is update_term at
    1.6e-6 (this batch removes most of P, so the two nearly agree); scaled_P 1.2e-5, 6 budgets.  (The same on K in the third
    product, Pn = B2 + D K^T, changes nothing: D = K S - Y is zero but for rounding.  On K or Y in the first: 9 - 11 budgets.)"""
    over, flat = _report("16-bit T in B2 T^T, forced_31", *_defect("forced_31", lambda i, n, X: truncate_to_16_bits(X)
                                                                  if (i, n) == (1, "B") else X))
    assert flat and "e_P" in over and "u_P" in over and "s_P" in over


def test_the_bound_sees_fp32_products_where_fp64_was_asked():
    """The same class on the streamed update: long_31 with fp32 products, held to the budget without them.  Seen: rel_err 4.5e-6 on
    dx and 7.3e-7 on P+, both inside the flat pair and 7 - 10 budgets; scaled_P 1.9e-5, 165 budgets: the measure that tells the
    two product modes apart by the widest margin."""
    prob, ref = fp.problem("long_31")
    stk = fm.stack(prob, ref, np.random.default_rng([99, 0]))
    dx, Pn = fm.update(stk, prob.P, prob.sigma, True, True)
    over, flat = _report("fp32 products, long_31", fp.metrics(dx, Pn, ref, prob.P), cases.streamed_budget("long_31", False))
    assert flat and "s_P" in over


def test_the_bound_sees_a_lost_tile_of_a_chain_product():
    """Sixteen columns of the K range of B2 = P - K Y^T lost (columns 160 - 175 of K zeroed as they are loaded) on forced_31.  This
    one the flat pair sees too: rel_err on P+ 7.0e-3.  scaled_P reads it at 5.0e-2 -- a twentieth of a sigma, 26000 budgets --
    and update_term at 7.8e-3; every measure on P+ catches it, scaled_P in the units that say what it costs."""
    def lose(i, n, X):
        if (i, n) == (0, "A"):
            X = X.copy()
            X[:, 160:176] = 0
        return X
    over, flat = _report("16 columns of K Y^T lost, forced_31", *_defect("forced_31", lose))
    assert "e_P" in over and "s_P" in over and "u_P" in over
