#!/usr/bin/env python3
"""Cost of the selection with and without the refinement of the triangulated points, and the A/B of refine_iters = 0
against the build in front of the feature, in ONE session on ONE box.

usage: select_refine_ab.py PARENT_ROOT [THIS_ROOT] [--runs 5] [--out FILE.md]

PARENT_ROOT is a checkout of the commit in front of the feature with its library built in place, THIS_ROOT this tree
(default).  A process loads one library and one package, so every measurement is a child process of the checkout it
measures, in alternating order, `--runs` each:

  parent      time_select(200) at (30, 2000, 10) and (30, 10000, 10) on the parent's build (one launch: k_select)
  this, 0     the same on this build with refine_iters = 0 (the same kernel, the same single launch)
  this, 8     refine_iters = 8  (k_select + k_select_refine)
  this, 24    refine_iters = 24

Batches: synth.make_problem(N, F, M, seed=0), make_tracks(seed 0, lost_fraction=1.0, pose_jitter=0.02), use_parallax off,
min_frames_tracked 2 -- every track is triangulated, so every track is a candidate of the refinement.
Medians and spreads (min .. max) of the per-process figures; the requirement is on refine_iters = 0 alone: its median lies
inside the parent's own run-to-run spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(30, 2000, 10), (30, 10000, 10)]

CHILD = r'''
import json, os, sys
root, iters, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
sys.path.insert(0, root)
import numpy as np
import msckf_amd
from msckf_amd import synth
from msckf_amd.api import UpdateEngine
fig = {}
for N, F, M in json.loads(sys.argv[4]):
    prob = synth.make_problem(N, F, M, seed=0)
    tracks = synth.make_tracks(prob, 0, lost_fraction=1.0, pose_jitter=0.02)
    kw = dict(use_parallax=False, min_frames_tracked=2)
    if iters >= 0:
        kw["refine_iters"] = iters                          # (the parent's SelectParams has no such field)
    with UpdateEngine(max_clones=N, max_features=F, max_track=M) as e:
        e.load(prob)
        e.set_tracks(tracks)
        e.run_select(synth.SelectParams(**kw), prob.K)
        e.time_select(50)                                   # warm
        us = e.time_select(200)
        rec = {"us": us}
        if iters > 0:
            sel, st = e.selection(), e.select_refine_stats()
            k = sel.refined
            rec.update(refined=int(k.sum()), trials_median=float(np.median(st["trials"][st["trials"] > 0])),
                       trials_max=int(st["trials"].max()), cost_ratio_median=float(np.median(st["cost1"][k] / st["cost0"][k])))
    fig["%d,%d,%d" % (N, F, M)] = rec
with open(out, "w") as f:
    json.dump(fig, f)
'''


def child(root, iters, out):
    env = {k: v for k, v in os.environ.items() if k != "MSCKF_LIB"}
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(root), str(iters), out, json.dumps(SIZES)], env=env,
                       capture_output=True, text=True, timeout=240, cwd=os.path.abspath(root))
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"child (refine_iters {iters}, {root}) ended with {r.returncode}")
    with open(out) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_root", metavar="PARENT_ROOT")
    ap.add_argument("this_root", metavar="THIS_ROOT", nargs="?", default=ROOT)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cols = [("parent", a.parent_root, -1), ("this, 0", a.this_root, 0), ("this, 8", a.this_root, 8), ("this, 24", a.this_root, 24)]
    fig = {key: [] for key, _, _ in cols}
    with tempfile.TemporaryDirectory() as tmp:
        for run in range(a.runs):                               # alternating processes
            for key, root, iters in cols:
                fig[key].append(child(root, iters, os.path.join(tmp, "fig.json")))
                print(run, key, fig[key][-1], flush=True)
    cell = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"
    text = ["## Selection (`time_select(200)`: k_select, and k_select_refine behind it when refine_iters > 0), microseconds per selection", "",
            f"Alternating processes in one session, {a.runs} runs each; median (min .. max).", "",
            "| (N, F, M) | parent build | this build, refine_iters 0 | refine_iters 8 | refine_iters 24 |", "|---|---|---|---|---|"]
    verdict, detail = [], []
    for N, F, M in SIZES:
        k = "%d,%d,%d" % (N, F, M)
        us = {key: [r[k]["us"] for r in fig[key]] for key in fig}
        text.append(f"| ({N}, {F}, {M}) | " + " | ".join(cell(us[key]) for key, _, _ in cols) + " |")
        inside = min(us["parent"]) <= statistics.median(us["this, 0"]) <= max(us["parent"])
        verdict.append(f"- ({N}, {F}, {M}): the refine_iters = 0 median lies {'inside' if inside else 'OUTSIDE'} the parent's own spread.")
        for key in ("this, 8", "this, 24"):
            r = fig[key][0][k]
            detail.append(f"- ({N}, {F}, {M}), {key.split(', ')[1]} trials at most: {r['refined']} of {F} tracks refined, trials median "
                          f"{r['trials_median']:.0f} / max {r['trials_max']}, median cost after / before {r['cost_ratio_median']:.3f}")
    out = "\n".join(text + [""] + verdict + [""] + detail) + "\n"
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
