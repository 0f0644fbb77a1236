#!/usr/bin/env python3
"""A/B of two builds of the library around the robust per-view weights (msckf_set_robust, k_robust), in ONE session on ONE box.

usage: view_robust_ab.py PARENT_ROOT [THIS_ROOT] [--runs 5] [--out FILE.md]

PARENT_ROOT is a checkout of the commit in front of the feature with its library built in place, THIS_ROOT this tree
(default).  A process loads one library and one package, so every measurement is a child process of the checkout it measures:

  bits   the goldens cfg2_A, edge_mixed_spans, edge_long_tracks, edge_null_pose through the one-shot call and through
         load / run on both builds, the option off: dx, P_new and the mask compared with np.array_equal
  cost   the K1-K4 stage (run_timed(stages=True), the `feature` figure) at (30, 2000, 10) and (30, 10000, 10) on batches with
         10 % gross outliers (400 px, one view of the track): parent and this build with the option off, this build with
         Huber (k = 1.345, w_min = 0.05) on, in alternating processes, `--runs` each; medians and the spread (min .. max)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ["cfg2_A", "edge_mixed_spans", "edge_long_tracks", "edge_null_pose"]
SIZES = [(30, 2000, 10), (30, 10000, 10)]

CHILD = r'''
import json, os, sys
root, mode, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import msckf_amd
from msckf_amd import synth
from msckf_amd.api import UpdateEngine
if mode == "bits":
    from conftest import load_golden
    res = {}
    for name in sys.argv[4:]:
        prob, _ = load_golden(name)
        M = int(np.diff(prob.view_ptr).max())
        with UpdateEngine(max_clones=prob.N, max_features=max(prob.F, 1), max_track=max(M, 2)) as e:
            one = e.update_problem(prob)
            e.load(prob); e.run()
            two = e.result()
        res[name + "/oneshot/dx"], res[name + "/oneshot/P"], res[name + "/oneshot/acc"] = one.dx, one.P_new, one.accepted
        res[name + "/resident/dx"], res[name + "/resident/P"], res[name + "/resident/acc"] = two.dx, two.P_new, two.accepted
    np.savez(out, **res)
else:
    fig = {}
    for N, F, M in json.loads(sys.argv[4]):
        prob = synth.make_problem(N, F, M, seed=0, outlier_fraction=0.1, outlier_px=400.0)
        with UpdateEngine(max_clones=N, max_features=F, max_track=M) as e:
            if mode == "cost_r":
                e.set_robust("huber", 1.345, 0.05)
            e.load(prob)
            e.run_timed(50, stages=True)                       # warm
            _, st = e.run_timed(200, stages=True)
            acc = int(e.result().accepted.sum())
            down = e.view_weights()["n_down"] if mode == "cost_r" else 0
        fig["%d,%d,%d" % (N, F, M)] = [st[0], acc, down]
    with open(out, "w") as f:
        json.dump(fig, f)
'''


def child(lib, mode, out, *args):
    env = {k: v for k, v in os.environ.items() if k != "MSCKF_LIB"}
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(lib), mode, out, *args], env=env, capture_output=True, text=True,
                       timeout=240, cwd=os.path.abspath(lib))
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"child ({mode}, {lib}) ended with {r.returncode}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib", metavar="PARENT_ROOT")
    ap.add_argument("this_lib", metavar="THIS_ROOT", nargs="?", default=ROOT)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-bits", action="store_true")
    a = ap.parse_args()
    import numpy as np
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        if not a.skip_bits:
            pa, th = os.path.join(tmp, "parent.npz"), os.path.join(tmp, "this.npz")
            child(a.parent_lib, "bits", pa, *GOLDENS)
            child(a.this_lib, "bits", th, *GOLDENS)
            zp, zt = np.load(pa), np.load(th)
            bad = [k for k in zp.files if not np.array_equal(zp[k], zt[k])]
            lines.append("## Option off against the parent build, bit for bit")
            lines.append("")
            for g in GOLDENS:
                same = not any(k.startswith(g + "/") for k in bad)
                lines.append(f"- `{g}`: dx, P_new, accepted of the one-shot call and of load / run: {'equal (np.array_equal)' if same else 'DIFFERENT'}")
            lines.append("")
            print("\n".join(lines), flush=True)
            if bad:
                raise SystemExit("differs from the parent: " + ", ".join(bad))
        fig = {"parent": [], "this": [], "this, Huber": []}
        for run in range(a.runs):                               # alternating processes
            for key, lib, mode in (("parent", a.parent_lib, "cost"), ("this", a.this_lib, "cost"), ("this, Huber", a.this_lib, "cost_r")):
                out = os.path.join(tmp, "cost.json")
                child(lib, mode, out, json.dumps(SIZES))
                with open(out) as f:
                    fig[key].append(json.load(f))
                print(run, key, fig[key][-1], flush=True)
    cost = ["## K1-K4 stage (`run_timed(stages=True)`, `feature`), microseconds", "",
            f"Batches with 10 % gross outliers.  Alternating processes in one session, {a.runs} runs each of 200 timed pipelines; median (min .. max).", "",
            "| (N, F, M) | parent | this build, option off | this build, Huber on | accepted off -> Huber | views down-weighted |", "|---|---|---|---|---|---|"]
    verdict = []
    for N, F, M in SIZES:
        k = "%d,%d,%d" % (N, F, M)
        col = {key: [r[k][0] for r in fig[key]] for key in fig}
        cell = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"
        cost.append(f"| ({N}, {F}, {M}) | {cell(col['parent'])} | {cell(col['this'])} | {cell(col['this, Huber'])} | "
                    f"{fig['this'][0][k][1]} -> {fig['this, Huber'][0][k][1]} | {fig['this, Huber'][0][k][2]} |")
        inside = min(col["parent"]) <= statistics.median(col["this"]) <= max(col["parent"])
        verdict.append(f"- ({N}, {F}, {M}): with the option off the median lies {'inside' if inside else 'OUTSIDE'} the parent's own spread.")
    text = "\n".join(lines + cost + [""] + verdict) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
