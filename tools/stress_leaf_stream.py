#!/usr/bin/env python3
"""Stress of the band plan's single K5-K7 launch (k_leaf_root_gain): seeded batches of the shapes that take it (N = 10 - 30,
200 - 2000 tracks of up to 10 views, uniform or ragged, 10 % outliers) in rotation through the one-shot call.  Every call must
match the oracle (1e-8 relative on dx and P+, the same accepted mask) and equal, bit for bit,
the first result of its batch; the count of calls that ran the single launch (k5_launches == 1) is reported (a batch whose
groups need more than eight leaves, or a second merge level, keeps the separate launches).
usage: stress_leaf_stream.py [calls] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import msckf_amd  # noqa: F401
from msckf_amd import synth
from msckf_amd.api import UpdateEngine
from oracle import msckf_oracle as oracle

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


batches = []
for k in range(16):
    N = int(rng.choice([10, 20, 30, 30]))
    F = int(rng.choice([300, 500, 1000, 2000, 2000]))
    M = int(rng.integers(4, min(N, 10) + 1))
    batches.append(synth.make_problem(N, F, M, seed=int(rng.integers(1 << 30)), variable_tracks=bool(k % 2),
                                      outlier_fraction=0.1, outlier_px=300.0))
refs = [oracle.update(b, dense_noise=False) for b in batches]
first = [None] * len(batches)
worst, bad, fused = 0.0, 0, 0
t0 = time.time()
with UpdateEngine(max_clones=30, max_features=2048, max_track=10) as eng:
    for i in range(calls):
        b = int(rng.integers(len(batches)))
        r = eng.update_problem(batches[b])
        fused += r.stats.get("k5_launches") == 1
        e = max(rel(r.dx, refs[b]["dx"]), rel(r.P_new, refs[b]["P_new"]))
        worst = max(worst, e)
        ok = r.status == refs[b]["status"] and np.array_equal(r.accepted, refs[b]["accepted"]) and e < 1e-8
        if first[b] is None:
            first[b] = r
        elif not (np.array_equal(r.dx, first[b].dx) and np.array_equal(r.P_new, first[b].P_new)):
            ok = False
        if not ok:
            bad += 1
            print(f"call {i} batch {b} (N={batches[b].N}, F={batches[b].F}): status {r.status}, rel err {e:.2e}", flush=True)
print(f"{calls} calls over {len(batches)} batches in {time.time() - t0:.0f} s: {bad} wrong, {fused} on the single K5-K7 launch, "
      f"worst rel err vs the oracle {worst:.2e}")
sys.exit(1 if bad else 0)
