#!/usr/bin/env python3
"""What priors on the tracks' points cost (msckf_set_point_priors, k_feature_prior), on the GPU, in ONE process.

usage: point_priors_cost.py [--rounds 7] [--iters 200] [--out profiles/point_priors.md]

Resident runs of (30, 2000, 10): the batch is loaded once; 0 %, 10 % and 100 % of its tracks carry a prior (Sigma_p with
principal standard deviations of 1 cm .. 30 cm on rotated axes, mean = p_lin + L z), alternated round after round behind a
warm-up; every cell is `run_timed(iters, stages=True)`: the whole pipeline and its K1-K4 stage per run, microseconds.  The
0 % setting is the engine with the priors cleared, so its repeated rounds give the spread the other figures are read against.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZE = (30, 2000, 10)
FRACTIONS = (0.0, 0.1, 1.0)


def draw(prob, fraction, seed=1):
    import numpy as np
    from msckf_amd import synth
    rng = np.random.default_rng(seed)
    F = prob.F
    has = np.zeros(F, dtype=np.uint8)
    has[rng.permutation(F)[:int(round(fraction * F))]] = 1
    mean, cov = np.zeros((F, 3)), np.zeros((F, 3, 3))
    for j in np.nonzero(has)[0]:
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        L = Q * np.exp(rng.uniform(np.log(0.01), np.log(0.30), 3))
        C = L @ L.T
        cov[j] = (C + C.T) / 2
        mean[j] = prob.idp_base[j] + prob.idp_m[j] / prob.idp_rho[j] + L @ rng.standard_normal(3)
    return synth.PointPriors(has, mean, cov)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_priors.md"))
    a = ap.parse_args()
    import msckf_amd  # noqa: F401
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    N, F, M = SIZE
    prob = synth.make_problem(N, F, M, seed=0)
    priors = {f: (draw(prob, f) if f > 0 else None) for f in FRACTIONS}
    total = {f: [] for f in FRACTIONS}
    feat = {f: [] for f in FRACTIONS}
    info = {}
    with UpdateEngine(max_clones=N, max_features=F, max_track=M) as e:
        e.load(prob)
        for f in FRACTIONS:                                     # warm-up: every setting once (plans, allocations)
            e.set_point_priors(priors[f])
            e.run_timed(50, stages=True)
        for r in range(a.rounds):
            for f in FRACTIONS:
                e.set_point_priors(priors[f])
                e.run()                                         # (the setting's plan is made in front of its first run: not timed)
                e.sync()
                ms, st = e.run_timed(a.iters, stages=True)
                total[f].append(ms * 1000.0 / a.iters)
                feat[f].append(st[0])
                res = e.result()
                info[f] = (int(res.accepted.sum()), res.stats["stacked_rows"])
                print(r, f, f"{total[f][-1]:.1f} us, K1-K4 {feat[f][-1]:.1f} us", flush=True)
    cell = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"
    lines = ["# Priors on the tracks' points: cost on the GPU (`tools/point_priors_cost.py`)", "",
             f"Resident runs of ({N}, {F}, {M}), one process, one loaded batch; the three settings alternated for {a.rounds} rounds behind a",
             f"warm-up, {a.iters} back-to-back pipelines per cell (`run_timed(stages=True)`).  Microseconds per run: median (min .. max).",
             "The 0 % column is the engine with the priors cleared: its spread is what the others are read against.", "",
             "| tracks with a prior | whole pipeline | K1-K4 stage | accepted | stacked rows |", "|---|---|---|---|---|"]
    for f in FRACTIONS:
        lines.append(f"| {100 * f:.0f} % | {cell(total[f])} | {cell(feat[f])} | {info[f][0]} | {info[f][1]} |")
    base = statistics.median(total[0.0])
    lines += ["", f"Spread of the repeated 0 % runs: {min(total[0.0]):.1f} .. {max(total[0.0]):.1f} us "
              f"({100 * (max(total[0.0]) - min(total[0.0])) / base:.1f} % of the median)."]
    for f in FRACTIONS[1:]:
        lines.append(f"{100 * f:.0f} % of the tracks with a prior: {statistics.median(total[f]) - base:+.1f} us on the pipeline, "
                     f"{statistics.median(feat[f]) - statistics.median(feat[0.0]):+.1f} us on K1-K4 (medians).")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
