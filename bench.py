#!/usr/bin/env python3
"""bench.py -- MSCKF measurement-updates/sec on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A "step" is one complete measurement update (K1..K7: per-feature Jacobian stack,
nullspace projection, chi-square gate, QR compression, gain, Joseph covariance
update) of ONE filter over one synthetic feature batch.

A plain run does only what the headline figure needs: it sets up, warms up, times
the K steps, writes --dump-outputs and prints ONE JSON line with the contract keys
(`metric`, `value`, `unit`, `ms_per_step`, ...).  Everything else below is measured
only with --full.

N = 1 : BASELINE.json configs[2] (headline: N=30 clones, 2000 features, track 10,
        fp64).  `value` is the metric BASELINE.md / SURVEY 8(d) define: the complete
        drop-in call (host arrays in -> dx, P+, mask on the host: sort, plan, PCIe both
        ways), K steps over FOUR DIFFERENT batches in rotation (seeds 0..3), so that
        the K5 plan cache misses on every call as it does in a filter that gets new
        tracks every frame.  With --full: `value_resident` is the rate with state,
        sorted tracks and plan resident in HBM (HIP events over the same number of
        steps), and `value_host_inclusive_cache_hit` the drop-in call on a repeated
        batch.  The same line carries one row per other single-GPU config (configs[1],
        the north-star target (30, 10000, 10), configs[3] on one GPU, configs[4] in fp64
        and with fp32 storage, a long-span batch, a 10 %-outlier batch) with its own
        roofline fractions, `roofline` for the dominant kernel group (K5) and
        `cpu_baseline`.
N > 1 : (launched by torch.distributed.run, one rank per GPU; only RANK / LOCAL_RANK /
        WORLD_SIZE are read -- the exchange is librccl behind the C-ABI, no PyTorch)
        the feature-sharded update of BASELINE.json configs[3]: `value` = updates/s of
        the 8000-feature update split over the N ranks ("scaling": "strong"), ONE RCCL
        gather of the compressed group records to rank 0, serial gain there, ONE RCCL
        broadcast of status | dx | P+ | gate bytes.  With --full the same update
        unsharded on one GPU and the weak-scaling figure (2000 features per rank) ride
        in the same line.

Rank 0 prints ONE JSON line.  The oracle (oracle/msckf_oracle.py) is only timed
as the CPU baseline (--full); it is never on the measured GPU path.

--dump-outputs DIR: rank 0 writes what the timed path returned on its last timed
step (status, dx, P_new, accepted; the strong case at N > 1) as DIR/<name>.npy in
float64.  The batches are seeded, so two builds run with the same arguments can be
compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
FP64_PEAK_TFLOPS = 78.6        # MI355X FP64 vector = matrix peak (AMD public; measured 77.2 TF with v_mfma_f64_16x16x4_f64,
                               # tools/ubench/f64_tput.hip)
FP32_PEAK_TFLOPS = 157.3       # MI355X_MICROARCH.md: FP32 vector = matrix peak


def algorithmic_costs(N, F, M, s=8, lens=None):
    """Canonical per-update bytes / flops of the reference's dense formulation,
    SURVEY.md section 8(d) (all features accepted); s = bytes per stored scalar.
    `lens` (views per feature) replaces the uniform track length M for ragged batches."""
    d, dc = 15 + 6 * N, 6 * N
    Mv = np.full(F, M, dtype=np.float64) if lens is None else np.asarray(lens, dtype=np.float64)
    qv = np.maximum(2 * Mv - 3, 1)
    m = float(qv.sum())
    peak = (FP64_PEAK_TFLOPS if s == 8 else FP32_PEAK_TFLOPS) * 1e12
    bytes_inputs = s * (float((2 * Mv + 7).sum()) + 24 * N + 2 * d * d + d) + 4 * float(Mv.sum()) + F
    bytes_stack = m * (d + 1) * s                           # written once (K4), read once (K5)
    fl_A = float((200 * Mv + 36 * Mv + 24 * Mv * (6 * Mv + 1) + 2 * qv * (6 * Mv) ** 2 + 12 * qv * qv * Mv + qv ** 3 / 3 + 2 * qv * qv).sum())
    fl_B = 2 * m * dc * dc - (2.0 / 3.0) * dc ** 3 + 4 * m * dc
    fl_C = 6 * dc * d * d + 4 * dc * dc * d + (2.0 / 3.0) * dc ** 3 + 4 * d ** 3
    t_A = (bytes_inputs + bytes_stack) / (HBM_PEAK_GBS * 1e9)
    t_B = fl_B / peak
    t_C = fl_C / peak
    return dict(bytes=bytes_inputs + 2 * bytes_stack, flops_A=fl_A, flops_B=fl_B, flops_C=fl_C,
                bytes_A=bytes_inputs + bytes_stack, t_roof_s=t_A + t_B + t_C, t_A=t_A, t_B=t_B, t_C=t_C, rows=m)


def headline_pmc_file():
    """The committed PMC summary of the HEADLINE workload: profiles/rNN_pmc.json of the highest round (the other
    workloads' files carry a tag behind the round: rNN_ns_pmc.json, rNN_cfg4_pmc.json, ...)."""
    import glob
    import re
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json")):
        m = re.fullmatch(r"r(\d+)_pmc\.json", os.path.basename(f))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), f)
    return best[1] if best else None


def pmc_traffic(kernel_prefixes):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes
    (profiles/*_pmc.json: FETCH_SIZE and WRITE_SIZE collected in separate --pmc runs of this
    same command; raw counters, see the note in profiles/*_summary.md).  None if absent."""
    f = headline_pmc_file()
    if not f:
        return None
    d = json.load(open(f))
    tot, calls = 0.0, 0
    for name, k in d["kernels"].items():
        if any(pfx in name for pfx in kernel_prefixes) and k.get("fetch_kb") is not None and k.get("write_kb") is not None:
            tot += (k["fetch_kb"] + k["write_kb"]) * 1024.0 * k["calls"]
            calls += k["calls"]
    return tot / calls if calls else None


def pmc_executed_flops(kernel_prefixes):
    """FP64 flops the kernels EXECUTE per launch, from the committed SQ pass of the same command (profiles/*_pmc.json):
    SQ_INSTS_VALU_FMA_F64 counts wavefront instructions, 64 lanes x 2 flop each.  None if absent."""
    f = headline_pmc_file()
    if not f:
        return None
    files = [f]
    d = json.load(open(f))
    tot, calls = 0.0, 0
    for name, k in d["kernels"].items():
        v = k.get("SQ_INSTS_VALU_FMA_F64")
        if any(pfx in name for pfx in kernel_prefixes) and v is not None:
            tot += float(v) * 128.0 * k["calls"]
            calls += k["calls"]
    return (tot / calls, os.path.basename(files[-1])) if calls else None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, status, dx, P_new, accepted):
    """--dump-outputs: one DIR/<name>.npy (float64) per array of an update's result.  An array that would take the total
    past DUMP_LIMIT_BYTES is written as a sample of its flattened entries: the same seeded positions for the same shape,
    so dumps of two builds still compare entry for entry."""
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_LIMIT_BYTES - 4096                          # room for the four .npy headers
    for name, a in (("status", [status]), ("dx", dx), ("accepted", accepted), ("P_new", P_new)):
        a = np.asarray(a, dtype=np.float64)
        if a.nbytes > left:
            keep = np.sort(np.random.default_rng(0).choice(a.size, left // a.itemsize, replace=False))
            a = a.reshape(-1)[keep]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes


def blas_threads():
    try:                                                    # threads the BLAS / LAPACK calls of the oracle may use
        from threadpoolctl import threadpool_info
        return max([int(p.get("num_threads", 1)) for p in threadpool_info()] or [1])
    except Exception:
        return os.cpu_count()


def cpu_baseline(prob, budget_s=12.0, dense_noise=False, max_reps=10):
    """The oracle (NumPy restatement of the reference path) on this box's host cores: reference-faithful
    per-feature Python loop, SVD nullspace, np.linalg.qr, explicit inverses, Joseph form.
    dense_noise=True is BASELINE.md section 3 mode (i): with the reference's dense sigma^2 * eye(m)
    (MSCKF.py:589) and Q^T R_o Q (:598); False is mode (ii), R_n = sigma^2 I analytically."""
    from oracle import msckf_oracle as oracle
    np.linalg.qr(np.random.default_rng(0).standard_normal((400, 60)))      # LAPACK warm-up
    ts, out = [], None
    t_all = time.perf_counter()
    while len(ts) < max_reps and (not ts or time.perf_counter() - t_all < budget_s):
        t0 = time.perf_counter()
        out = oracle.update(prob, dense_noise=dense_noise)
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    cpu_baseline.last_samples = [float(x) for x in ts]
    return out, t, len(ts), float(sum(ts))


def time_config(N, F, M, steps, warmup, dtype="f64", device=0, host_reps=10, rotate=4, make=None):
    """One single-GPU config: resident rate (HIP events over `steps` back-to-back pipelines), per-stage device
    times, the rate of the complete drop-in call over `rotate` different batches in rotation (the plan cache
    misses on every call, as in a filter) and on one repeated batch (cache hit), roofline fractions.
    `make(seed)` builds the batches (default: the SURVEY 8(d) recipe)."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    make = make or (lambda sd: synth.make_problem(N, F, M, seed=sd))
    probs = [make(sd) for sd in range(max(1, rotate))]
    prob = probs[0]
    F = prob.F
    s = 8 if dtype == "f64" else 4
    costs = algorithmic_costs(N, F, M, s, lens=np.diff(prob.view_ptr))
    with UpdateEngine(max_clones=N, max_features=max(p.F for p in probs), max_track=max(M, 2), device=device, dtype=dtype) as eng:
        eng.load(prob)
        for _ in range(warmup):
            eng.run()
        eng.sync()
        t0 = time.perf_counter()
        ms_ev, _ = eng.run_timed(steps)
        eng.sync()
        wall = time.perf_counter() - t0
        _, stages = eng.run_timed(min(steps, 30), stages=True)
        res = eng.result()
        for _ in range(2):
            one = eng.update_problem(prob)
        t1 = time.perf_counter()
        for _ in range(host_reps):
            one = eng.update_problem(prob)
        hit_s = (time.perf_counter() - t1) / host_reps
        for i in range(len(probs)):                          # warm the allocations of every batch shape
            eng.update_problem(probs[i])
        t1 = time.perf_counter()
        for i in range(host_reps):
            one_r = eng.update_problem(probs[i % len(probs)])
        host_s = (time.perf_counter() - t1) / host_reps
        one = eng.update_problem(prob)
    us = 1e3 * ms_ev / steps
    peak = FP64_PEAK_TFLOPS if dtype == "f64" else FP32_PEAK_TFLOPS
    row = {
        "workload": f"N={N} clones, F={F} features, track={M}, {'fp64' if dtype == 'f64' else 'fp32 storage'}",
        "dtype": dtype,
        "updates_per_s": 1e6 / us, "us_per_update": us, "wall_us_per_update": 1e6 * wall / steps,
        "host_inclusive_updates_per_s": 1.0 / host_s, "host_inclusive_us": 1e6 * host_s,
        "host_inclusive_cache_hit_updates_per_s": 1.0 / hit_s, "host_inclusive_cache_hit_us": 1e6 * hit_s,
        "host_inclusive_protocol": f"{host_reps} calls over {len(probs)} different batches in rotation (plan cache misses)",
        "roofline_frac_pipeline_host_inclusive_canonical": costs["t_roof_s"] / host_s,
        "stages_us": {"feature_K1_K4": stages[0], "qr_K5": stages[1], "gain_K6_K7": stages[2]},
        "features": int(F), "accepted": int(res.accepted.sum()), "stacked_rows": int(one.stats.get("stacked_rows", 0)),
        "k5_launches": int(one.stats.get("k5_launches", 0) or one.stats.get("n_levels", 0)), "leaves": int(one.stats.get("n_leaves", 0)),
        "host_prep_us": one.stats.get("us_host_prep"), "h2d_us": one.stats.get("us_h2d"), "d2h_us": one.stats.get("us_d2h"),
        # every fraction below prices the CANONICAL bytes / flops of SURVEY 8(d) (the reference's dense formulation) against the
        # measured time; the kernels execute far fewer flops than that (band QR, D - V Z gate), so a stage fraction can pass 1
        "roofline_frac_pipeline_canonical": costs["t_roof_s"] * 1e6 / us,
        "t_roof_us": costs["t_roof_s"] * 1e6,
        "roofline_frac_K1_K4_hbm_canonical": costs["t_A"] * 1e6 / stages[0],
        "roofline_frac_K5_canonical": costs["t_B"] * 1e6 / stages[1],
        "roofline_frac_K6_K7_canonical": costs["t_C"] * 1e6 / max(stages[2], 1e-3),
        "stage_note": "K5 and K6-K7 share one launch where the root is a k_sweep (k_root_gain): K6-K7 is what trails the sweep's last "
                      "published row (in-kernel time stamps), K5 the rest",
        "K5_tflops_canonical": costs["flops_B"] / (stages[1] * 1e-6) / 1e12, "peak_tflops": peak,
        "hbm_gbs_algorithmic": costs["bytes"] / (us * 1e-6) / 1e9,
    }
    return prob, res, one, row, costs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--clones", type=int, default=30)
    ap.add_argument("--features", type=int, default=2000, help="features per GPU")
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline too: resident rate, stage times, rooflines, the other configs, "
                         "f1-f4 and the CPU baseline at one GPU; the unsharded run and weak scaling at N > 1")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra-configs", action="store_true", help="with --full: no other configs (profiling runs)")
    ap.add_argument("--no-mode-i-headline", action="store_true",
                    help="with --full: skip the one-minute dense-eye CPU baseline at the headline")
    ap.add_argument("--force-dist", action="store_true", help="run the sharded code path even at world size 1")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the result of the last timed step to DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        args.gpus = world
    N, Fg, M = args.clones, args.features, args.track

    use_dist = world > 1 or args.force_dist
    import msckf_amd  # noqa: F401
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine

    if use_dist:
        line = bench_sharded(args, world, rank, local_rank)
        if rank == 0:
            print(json.dumps(line), flush=True)
        return

    # ---- the timed region of the contract: W warm-up + EXACTLY K complete drop-in calls (host arrays in -> dx, P+,
    #      mask on the host) over four different batches in rotation; every call blocks until its results are on the host
    probs4 = [synth.make_problem(N, Fg, M, seed=sd) for sd in range(4)]
    with UpdateEngine(max_clones=N, max_features=Fg, max_track=max(M, 2), device=local_rank) as eng:
        for i in range(max(args.warmup, 4)):
            eng.update_problem(probs4[i % 4])
        eng.sync()
        t0 = time.perf_counter()
        for i in range(args.steps - 1):
            eng.update_problem(probs4[i % 4])
        last = eng.update_problem(probs4[(args.steps - 1) % 4])    # the last timed call: what --dump-outputs writes
        eng.sync()
        call_s = (time.perf_counter() - t0) / args.steps
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last.status, last.dx, last.P_new, last.accepted)
    line = {
        "metric": "MSCKF measurement-updates/sec (N=30 clones, 2000 features, track=10)",
        "value": 1.0 / call_s,
        "unit": "updates/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": call_s * 1e3,
        "higher_is_better": True,
        "scaling": "none",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"N={N} clones, F={Fg} features, track={M}, fp64",
                   "unit_definition": "one 2000-feature measurement update (K1-K7)", "seeds": [0, 1, 2, 3],
                   "value_definition": "the metric of BASELINE.md / SURVEY 8(d): the complete drop-in call, host arrays in -> dx, P+, "
                                       "mask on the host (sort, plan, PCIe both ways, K1-K7), `steps` calls over four different "
                                       "batches in rotation so that the K5 plan cache misses on every call"},
    }
    if args.full:
        full_single_gpu(args, line, call_s, local_rank)
    else:
        print(json.dumps(line), flush=True)


def full_single_gpu(args, line, call_s, local_rank):
    """--full at one GPU: everything beside the headline figure, measured after its timed steps and added to `line`, which
    emit() prints (the detail goes to bench_detail.json)."""
    from msckf_amd import synth, _ffi
    from msckf_amd.api import UpdateEngine
    N, Fg, M = args.clones, args.features, args.track
    prob, res, one, head, costs = time_config(N, Fg, M, args.steps, args.warmup, device=local_rank, host_reps=20)
    stats = one.stats
    us_step = head["us_per_update"]
    us_qr = head["stages_us"]["qr_K5"]
    n_lv = max(1, head["k5_launches"])
    line["config"]["value_definition"] += ("; value_resident = K1-K7 with state, sorted tracks and plan resident in HBM, HIP events "
                                           "over `steps` pipelines")
    line.update({
        "value_resident": head["updates_per_s"],
        "ms_per_step_resident": us_step * 1e-3,
        "value_host_inclusive_cache_hit": head["host_inclusive_cache_hit_updates_per_s"],
        "host_inclusive_updates_per_s": 1.0 / call_s,
        "host_inclusive_breakdown_us": {"call": call_s * 1e6, "call_cache_hit": head["host_inclusive_cache_hit_us"],
                                        "device_pipeline": us_step,
                                        "host_sort_plan": head["host_prep_us"], "h2d": head["h2d_us"], "d2h": head["d2h_us"]},
    })
    k5_names = ("k_lsweep<", "k_sweep<", "k_wsweep<", "k_root_gain<", "k_root_gain_m<")
    ex = pmc_executed_flops(k5_names)
    line["roofline"] = {
        "kernel": "K5 QR compression: k_lsweep leaves + group merges + the root sweep (%d launches per update; the last merge "
                  "level and the root share k_root_gain's launch, which also holds K6-K7, whose trailing part is not counted here)" % n_lv,
        "bound": "fp64_valu", "unit": "TFLOP/s",
        "achieved": costs["flops_B"] / (us_qr * 1e-6) / 1e12,
        "peak": FP64_PEAK_TFLOPS,
        "frac": costs["flops_B"] / (us_qr * 1e-6) / 1e12 / FP64_PEAK_TFLOPS,
        "frac_canonical": costs["flops_B"] / (us_qr * 1e-6) / 1e12 / FP64_PEAK_TFLOPS,
        "traffic": pmc_traffic(k5_names),
        "flops_per_launch": costs["flops_B"] / n_lv,
        "avg_launch_us": us_qr / n_lv,
        "flops_model": "`achieved` / `frac` price the CANONICAL flops of a dense Householder QR of the m x 6N stack (SURVEY 8d: "
                       "2 m dc^2 - 2/3 dc^3 + 4 m dc) against the measured K5 time; `executed_flops` is what the kernels really "
                       "issue (SQ_INSTS_VALU_FMA_F64 x 128 per launch from the committed PMC pass): the band pipeline factors "
                       "windows of 6 x track columns only",
        "executed_flops_per_launch": ex[0] if ex else None,
        "executed_tflops": (ex[0] * n_lv / (us_qr * 1e-6) / 1e12) if ex else None,
        "frac_executed": (ex[0] * n_lv / (us_qr * 1e-6) / 1e12 / FP64_PEAK_TFLOPS) if ex else None,
        "executed_from": ex[1] if ex else None,
    }
    line["pipeline_roofline"] = {"t_roof_us": costs["t_roof_s"] * 1e6, "t_measured_us": us_step,
                                 "frac_canonical": costs["t_roof_s"] * 1e6 / us_step,
                                 "frac_host_inclusive_canonical": costs["t_roof_s"] / call_s,
                                 "hbm_gbs_algorithmic": costs["bytes"] / (us_step * 1e-6) / 1e9}
    line["k5_launches"] = n_lv
    line["stages_us"] = dict(head["stages_us"], hip_event_ms_per_step=us_step * 1e-3)
    line["accepted"] = head["accepted"]
    line["plan"] = {"leaves": stats.get("n_leaves"), "levels": stats.get("n_levels"),
                    "host_prep_us": stats.get("us_host_prep"), "h2d_us": stats.get("us_h2d")}

    # ---- the other single-GPU configs, same protocol, fewer steps -------------------------------------
    rows = [dict(head, config="configs[2] headline")]
    if not args.no_extra_configs:
        extra = [("configs[1]", 20, 500, 8, "f64", 100, None), ("north-star target", 30, 10000, 10, "f64", 50, None),
                 ("configs[3] on one GPU", 30, 8000, 10, "f64", 50, None),
                 ("configs[4] in fp64", 50, 20000, 15, "f64", 20, None),
                 ("configs[4] fp32 storage + f32 MFMA P-update", 50, 20000, 15, "f32", 20, None),
                 # tracks of 2..30 consecutive clones (the reference's default window is 30 clones, MSCKF.py:45): tracks of more
                 # than 10 slots are split (two-level nullspace basis): their <= 10-slot blocks join the band pipeline
                 # of the others, their remainder rows go to K6-K7 as they are or through a merge tree of their own
                 ("long spans: N=30, 2000 features, track ~ U[2, 30]", 30, 2000, 30, "f64", 20,
                  lambda sd: synth.make_problem(30, 2000, 30, seed=sd, variable_tracks=True, min_track=2)),
                 ("spans <= 15: N=30, 2000 features, track ~ U[2, 15]", 30, 2000, 15, "f64", 50,
                  lambda sd: synth.make_problem(30, 2000, 15, seed=sd, variable_tracks=True, min_track=2)),
                 ("a few long tracks: N=30, 1990 ten-view + 10 thirty-view tracks", 30, 2000, 30, "f64", 50,
                  lambda sd: synth.few_long_tracks_problem(30, 2000, 10, 10, seed=sd)),
                 # a 50-clone window (MSCKFParameters.max_number_of_camera_states is a free parameter, MSCKF.py:45): long tracks are
                 # split there too (round 4's information form stopped at 31 clones); beside it the batch it is measured against
                 ("N=50, 2000 features, track=15 (90-column pipeline)", 50, 2000, 15, "f64", 30, None),
                 ("long spans at N=50: 2000 features, track ~ U[2, 31]", 50, 2000, 31, "f64", 20,
                  lambda sd: synth.make_problem(50, 2000, 31, seed=sd, variable_tracks=True, min_track=2)),
                 # (the reference's front end keeps at most 300 features per frame, main.py:199)
                 ("a frame of the reference's size: N=30, 300 features, track ~ U[2, 30], 10 % outliers", 30, 300, 30, "f64", 50,
                  lambda sd: synth.make_problem(30, 300, 30, seed=sd, variable_tracks=True, min_track=2, outlier_fraction=0.10, outlier_px=400.0)),
                 ("10 % gross outliers: N=30, 2000 features, track=10", 30, 2000, 10, "f64", 50,
                  lambda sd: synth.make_problem(30, 2000, 10, seed=sd, outlier_fraction=0.10, outlier_px=400.0))]
        for name, n, f, m, dt, st, mk in extra:
            try:
                _, _, _, row, _ = time_config(n, f, m, st, 5, dtype=dt, device=local_rank, host_reps=8, make=mk)
                rows.append(dict(row, config=name))
            except Exception as e:                           # a config that cannot run is reported, not hidden
                rows.append({"config": name, "error": repr(e)})
    line["configs"] = rows
    ns = [r for r in rows if r.get("config") == "north-star target" and "error" not in r]
    if ns:                                                   # BASELINE.json north_star: >= 10k features, 30 clones, >= 40 % of the roofline
        line["north_star_roofline"] = {"workload": ns[0]["workload"], "t_roof_us": ns[0]["t_roof_us"],
                                       "us_per_update_resident": ns[0]["us_per_update"],
                                       "frac": ns[0]["roofline_frac_pipeline_canonical"],
                                       "frac_host_inclusive": ns[0]["roofline_frac_pipeline_host_inclusive_canonical"],
                                       "model": "canonical bytes / flops of SURVEY 8(d): T_roof = bytes_A / 8 TB/s + flops_B / 78.6 TF + flops_C / 78.6 TF",
                                       "updates_per_s_resident": ns[0]["updates_per_s"],
                                       "updates_per_s_host_inclusive": ns[0]["host_inclusive_updates_per_s"]}

    # f1, reported beside the headline, never inside `value`: the selection +
    # triangulation kernel on the same tracks, and the fused select -> update pass.
    with UpdateEngine(max_clones=N, max_features=Fg, max_track=max(M, 2), device=local_rank) as eng:
        tracks = synth.make_tracks(prob, 0, lost_fraction=0.5)
        sp = synth.SelectParams(min_parallax_deg=8.0)
        eng.load(prob)
        eng.set_tracks(tracks)
        eng.run_select(sp, prob.K)
        us_sel = eng.time_select(50)
        eng.run()
        eng.sync()
        ms_masked, _ = eng.run_timed(50)                       # K1-K7 over the valid subset, HIP events
        us_fused = us_sel + ms_masked / 50 * 1e3
        t2 = time.perf_counter()
        eng.replan()                                           # tree over the valid features only (syncs)
        us_replan = (time.perf_counter() - t2) * 1e6
        eng.run()
        eng.sync()
        ms_replanned, _ = eng.run_timed(50)
        n_views = int(prob.view_ptr[-1])
        sel_bytes = n_views * (7 * 8 + 4) + prob.F * (3 * 4 + 1 + 7 * 8)
        line["select_f1"] = {"kernel": "k_select (get_valid_features)", "us_per_launch": us_sel,
                             "candidates": prob.F, "valid": int(eng.selection().valid.sum()),
                             "bytes_algorithmic": sel_bytes, "hbm_gbs_algorithmic": sel_bytes / (us_sel * 1e-6) / 1e9,
                             "fused_select_update_us": us_fused,
                             "replan_host_us": us_replan,
                             "fused_replanned_us": us_sel + us_replan + ms_replanned / 50 * 1e3}
        # f4: the association tests of the front end's matches against their tracks (k_assoc), blocking call:
        # upload of the matched keypoints, one launch, results back
        rng4 = np.random.default_rng(4)
        eng.load(prob)
        ends = prob.view_ptr[1:] - 1
        muv = prob.obs_uv[ends] + rng4.normal(0, 1.0, (prob.F, 2))
        Rc, tc = prob.cam_R[-1], prob.cam_t[-1] + np.array([0.15, 0.0, 0.0])
        for _ in range(3):
            a_res, _ = eng.associate(muv, Rc, tc, prob.K)
        t5 = time.perf_counter()
        for _ in range(50):
            a_res, _ = eng.associate(muv, Rc, tc, prob.K)
        us_assoc = (time.perf_counter() - t5) / 50 * 1e6
        assoc_bytes = int(prob.view_ptr[-1]) * 20 + prob.F * (16 + 5)
        line["associate_f4"] = {"kernel": "k_assoc (add_camera_measurements tests, MSCKF.py:332-412)",
                                "us_per_call_host_inclusive": us_assoc, "matches": prob.F, "kept": int((a_res == 0).sum()),
                                "match_views": int(prob.view_ptr[-1]), "bytes_algorithmic": assoc_bytes,
                                "hbm_gbs_algorithmic": assoc_bytes / (us_assoc * 1e-6) / 1e9}
        # the per-frame loop of a filter that keeps P in HBM (f2): new tracks in, K1-K7, dx out, P+ committed on the device,
        # poses of the corrected clones back in -- no covariance crosses PCIe.  Four different batches in rotation.
        probs_loop = [prob] + [synth.make_problem(N, Fg, M, seed=sd) for sd in (1, 2, 3)]
        eng.set_state(prob)

        def frame(p):
            eng.set_features(p)
            eng.run()
            dxv = np.empty(p.d)
            stt = _ffi.Stats()
            rc = eng._check(eng._lib.msckf_get_result(eng._h, _ffi.dptr(dxv), None, None, C.byref(stt)))
            if rc == 0:
                eng.commit_covariance()
            eng.set_poses(p.cam_R, p.cam_t)
            return dxv

        for i in range(8):
            frame(probs_loop[i % 4])
        t6 = time.perf_counter()
        for i in range(100):
            frame(probs_loop[i % 4])
        us_frame = (time.perf_counter() - t6) / 100 * 1e6
        line["resident_filter_loop"] = {
            "what": "set_features (new batch) -> run -> get_result(dx only) -> commit_covariance -> set_poses, covariance resident in HBM",
            "us_per_frame": us_frame, "updates_per_s": 1e6 / us_frame, "batches": 4}
        # f2 / f3: the covariance steps either side of the update on the resident P (host clock
        # around async launches + one sync; augment / remove include their pose upload and sync)
        rng = np.random.default_rng(0)
        eng.set_prior(prob.P, prob.gravity, prob.K, prob.sigma, prob.cam_R, prob.cam_t)
        Phi = np.eye(15) + 1e-3 * rng.standard_normal((15, 15))
        Qd = 1e-8 * np.eye(15)
        for _ in range(10):
            eng.propagate(Phi, Qd)
        eng.sync()
        t3 = time.perf_counter()
        for _ in range(200):
            eng.propagate(Phi, Qd)
        eng.sync()
        us_prop = (time.perf_counter() - t3) / 200 * 1e6
        J15 = np.zeros((6, 15)); J15[:3, :3] = np.eye(3); J15[3:, 12:] = np.eye(3)
        t4 = time.perf_counter()
        for _ in range(20):
            eng.remove_clones([0])
            eng.augment(J15, prob.cam_R[0], prob.cam_t[0])
        us_window = (time.perf_counter() - t4) / 20 * 1e6
        line["resident_f2_f3"] = {"propagate_us": us_prop, "remove_plus_augment_us": us_window,
                                  "clones": N, "bytes_per_propagate": (2 * 15 * prob.d * 2 + prob.d * prob.d * 2) * 8}

    # the CPU baseline runs last: its BLAS threads keep spinning and would disturb host-clocked numbers
    if not args.no_cpu_baseline:
        cores = blas_threads()
        ref, t, reps, tot = cpu_baseline(prob, budget_s=12.0)
        line["cpu_baseline"] = dict(
            value=1.0 / t, unit="updates/s", cores=cores, kind="port",
            sample=f"{reps} full updates of the headline workload (median {t:.2f} s each, {tot:.0f} s in all); "
                   "per-feature stage is a single-threaded Python loop, QR / products use the BLAS "
                   f"thread pool ({cores} threads, {os.cpu_count()} logical CPUs); mode (ii) of BASELINE.md 3: oracle with "
                   "R_n = sigma^2 I analytic instead of the reference's dense sigma^2*eye(m) (9.2 GB at this size)")
        line["cpu_baseline"]["sample_short"] = (f"{reps} full headline updates, median {t:.2f} s ({tot:.0f} s in all); oracle mode (ii): "
                                                f"R_n = sigma^2 I analytic; Python per-feature loop + BLAS pool of {cores} threads")
        line["cpu_baseline"]["samples_s"] = list(getattr(cpu_baseline, "last_samples", []))
        # the same update with the BLAS pool limited to 1 / 8 / 64 threads (rounds 1-3 read 1.000 +/- 0.0005 updates/s on
        # three different boxes: the un-quantised samples and this sweep say what the host is doing)
        try:
            from threadpoolctl import threadpool_limits
            sweep = []
            for nt in (1, 8, 64):
                if nt > (os.cpu_count() or 1):
                    continue
                with threadpool_limits(limits=nt):
                    _, t_nt, reps_nt, _ = cpu_baseline(prob, budget_s=5.0, max_reps=3)
                sweep.append({"blas_threads": nt, "median_s": t_nt, "samples_s": list(cpu_baseline.last_samples)})
            line["cpu_baseline"]["blas_thread_sweep"] = sweep
        except Exception as e:
            line["cpu_baseline"]["blas_thread_sweep"] = {"error": repr(e)}
        e_dx = float(np.linalg.norm(res.dx - ref["dx"]) / np.linalg.norm(ref["dx"]))
        e_P = float(np.linalg.norm(res.P_new - ref["P_new"]) / np.linalg.norm(ref["P_new"]))
        line["parity_vs_cpu_baseline"] = {"dx_rel": e_dx, "P_rel": e_P}
        # mode (i): reference-faithful WITH the dense sigma^2 * eye(m) (MSCKF.py:589, :598), where it fits: configs 1-2
        mode_i = []
        for name, n, f, m in (("configs[0]", 10, 50, 5), ("configs[1]", 20, 500, 8)):
            p = synth.make_problem(n, f, m, seed=0)
            _, t_i, reps_i, _ = cpu_baseline(p, budget_s=4.0, dense_noise=True, max_reps=7)
            _, t_ii, _, _ = cpu_baseline(p, budget_s=2.0, dense_noise=False, max_reps=7)
            mode_i.append({"config": name, "workload": f"N={n}, F={f}, track={m}", "rows": int(f * (2 * m - 3)),
                           "mode_i_dense_eye_updates_per_s": 1.0 / t_i, "mode_i_median_s": t_i, "reps": reps_i,
                           "mode_ii_updates_per_s": 1.0 / t_ii})
        line["cpu_baseline"]["mode_i"] = mode_i
        if not args.no_mode_i_headline:
            # the reference's own formulation at the headline: dense sigma^2 * eye(34000) (9.2 GB, MSCKF.py:589) and
            # Q^T R_o Q (:598) -- one update, about a minute of host time
            try:
                _, t_h, reps_h, _ = cpu_baseline(prob, budget_s=1.0, dense_noise=True, max_reps=1)
                line["cpu_baseline"]["mode_i_headline"] = {
                    "workload": f"N={N}, F={Fg}, track={M}", "rows": int(costs["rows"]), "updates_per_s": 1.0 / t_h,
                    "seconds": t_h, "reps": reps_h, "cores": cores,
                    "note": "reference-faithful mode (i) of BASELINE.md 3: dense R_o = sigma^2 eye(m), m = 34000"}
            except MemoryError as e:
                line["cpu_baseline"]["mode_i_headline"] = {"error": repr(e)}
    emit(line)


def emit(detail):
    """The ONE stdout line of the contract, kept under 4 KB (round 4's had grown to 20 KB and the driver's parser returned
    null): the contract keys, `roofline`, `cpu_baseline`, `north_star_roofline`, parity.  Everything else -- the per-config
    rows, stage times, thread sweeps, sample lists, f1 / f2 / f3 / f4 rows -- goes to bench_detail.json beside this file
    and, pretty-printed, to stderr (before the stdout line)."""
    try:
        with open(os.path.join(ROOT, "bench_detail.json"), "w") as fh:
            json.dump(detail, fh, indent=1)
    except OSError as e:
        print("bench_detail.json not written: %r" % (e,), file=sys.stderr)
    print(json.dumps(detail, indent=1), file=sys.stderr, flush=True)
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "value_resident", "ms_per_step_resident", "accepted")
    line = {k: detail[k] for k in keep if k in detail}
    line["config"] = {"workload": detail["config"]["workload"],
                      "value_definition": "complete drop-in call, host arrays in -> dx, P+, mask on the host (PCIe both ways), four "
                                          "batches in rotation; value_resident: K1-K7 with inputs resident in HBM (HIP events)"}
    r = detail["roofline"]
    line["roofline"] = {"kernel": "K5 QR compression (k_lsweep + merge levels + root sweep), %d launches/update" % detail["k5_launches"],
                        "bound": r["bound"], "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"],
                        "frac_executed": r.get("frac_executed"), "traffic": r.get("traffic"),
                        "flops_per_launch": r["flops_per_launch"], "avg_launch_us": r["avg_launch_us"],
                        "flops_model": "canonical dense-QR flops of SURVEY 8(d); frac_executed: SQ_INSTS_VALU_FMA_F64 of the committed PMC pass"}
    if "cpu_baseline" in detail:
        cb = detail["cpu_baseline"]
        line["cpu_baseline"] = {"value": cb["value"], "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                                "sample": cb["sample_short"]}
        line["parity_vs_cpu_baseline"] = detail.get("parity_vs_cpu_baseline")
    if "north_star_roofline" in detail:
        ns = detail["north_star_roofline"]
        line["north_star_roofline"] = {"workload": ns["workload"], "frac": ns["frac"], "frac_host_inclusive": ns["frac_host_inclusive"],
                                       "us": ns["us_per_update_resident"], "t_roof_us": ns["t_roof_us"]}
    line["pipeline_roofline"] = {k: detail["pipeline_roofline"][k] for k in ("t_roof_us", "t_measured_us", "frac_canonical",
                                                                            "frac_host_inclusive_canonical")}
    line["stages_us"] = {k: detail["stages_us"][k] for k in ("feature_K1_K4", "qr_K5", "gain_K6_K7")}
    line["detail"] = "bench_detail.json (also on stderr)"
    out = json.dumps(line)
    assert len(out) < 4096, len(out)
    print(out, flush=True)


def bench_sharded(args, world, rank, local_rank):
    """N > 1: one rank per GPU, exchange on librccl behind the C-ABI (msckf_comm_*, no PyTorch).  `value` is
    BASELINE.json configs[3] as written -- ONE 8000-feature update split over the ranks ("strong") --.  With --full the
    unsharded run on rank 0 and the weak figure (2000 features per rank, counted as 2000-feature update equivalents) ride
    in the same line."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import RcclShardedUpdate, exchange_unique_id
    N, Fg, M = args.clones, args.features, args.track
    os.environ.setdefault("NCCL_DEBUG_FILE", "/dev/stderr")      # RCCL's version banner must not land beside the JSON line
    id_base = "/tmp/msckf_rccl_id_%s_%s_%d" % (os.environ.get("MASTER_PORT", "0"), os.environ.get("TORCHELASTIC_RUN_ID", "x"),
                                               os.getppid())

    def run_case(F_total, steps, warmup, tag):
        prob = synth.make_problem(N, F_total, M, seed=0)
        eng = UpdateEngine(max_clones=N, max_features=F_total, max_track=max(M, 2), device=local_rank)
        uid = exchange_unique_id(eng, rank, world, id_base + tag)
        # librccl prints its version banner with plain printf at communicator creation: keep stdout for the ONE JSON line
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        try:
            drv = RcclShardedUpdate(eng, rank, world, uid, id_path=id_base + tag)
            drv.load(prob)                                   # every rank keeps its shard (and the state) resident
            drv.step()
            eng.sync()
        finally:
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)
        tbuf = drv.scratch                                   # a few doubles behind the exchange buffers

        def barrier():
            eng.comm_allreduce(tbuf, 1, "sum")
            eng.sync()

        for _ in range(warmup):
            drv.step()
        eng.sync()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            drv.step()                                       # compress -> RCCL gather -> merge + K6-K7 on rank 0 -> RCCL broadcast
        eng.sync()
        barrier()
        wall = time.perf_counter() - t0
        eng.comm_put(tbuf, np.array([wall]))
        eng.comm_allreduce(tbuf, 1, "max")
        eng.sync()
        seconds = float(eng.comm_get(tbuf, 1)[0])
        status, dx, P, acc, n_rej = drv.result()             # the same on every rank (shared result range)
        groups = drv.groups
        drv.close()
        eng.close()
        return seconds, groups, status, int(acc.sum()), n_rej, (dx, P, acc)

    # the same 8000-feature update on ONE GPU (rank 0's, unsharded, resident in HBM): what the strong-scaling figure is a
    # speed-up over.  The other ranks wait in the bootstrap of the first sharded case.
    one_gpu_us = None
    if rank == 0 and args.full:
        p8 = synth.make_problem(N, 8000, M, seed=0)
        with UpdateEngine(max_clones=N, max_features=8000, max_track=max(M, 2), device=local_rank) as e1:
            e1.load(p8)
            for _ in range(5):
                e1.run()
            e1.sync()
            ms1, _ = e1.run_timed(30)
            one_gpu_us = 1e3 * ms1 / 30
    s_seconds, s_groups, st2, s_acc, s_rej, s_out = run_case(8000, args.steps, args.warmup, "_strong")
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, st2, *s_out)
    if args.full:
        weak_steps = max(10, min(args.steps, 100))
        seconds, groups, st1, _, _, _ = run_case(Fg * world, weak_steps, min(args.warmup, 10), "_weak")
    line = None
    if rank == 0:
        line = {
            "metric": "MSCKF measurement-updates/sec (N=30 clones, 8000 features, track=10, feature-sharded)",
            "value": args.steps / s_seconds,
            "unit": "updates/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * s_seconds / args.steps,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"BASELINE.json configs[3]: N={N} clones, 8000 features in all, track={M}, fp64, feature-sharded "
                                   f"over {world} GPUs, 1 RCCL gather + 1 RCCL broadcast per update (librccl behind the C-ABI, "
                                   "no PyTorch); shards resident in HBM",
                       "exchange": "group triangles" if s_groups else "root blocks",
                       "unit_definition": "one 8000-feature measurement update (K1-K7)", "seed": 0},
            "status": [int(st2)],                            # one per case run: strong, then weak with --full
            "accepted": s_acc, "rejected": s_rej,
        }
    if rank == 0 and args.full:
        line["status"].append(int(st1))
        line.update({
            "one_gpu_same_workload": {"us_per_update": one_gpu_us, "updates_per_s": 1e6 / one_gpu_us,
                                      "what": "the unsharded 8000-feature update on rank 0's GPU, resident in HBM (HIP events)"},
            "speedup_vs_one_gpu": (args.steps / s_seconds) / (1e6 / one_gpu_us),
            "weak_scaling": {
                "workload": f"N={N} clones, {Fg} features per GPU ({Fg * world} per update), track={M}, fp64",
                "updates_per_s": weak_steps / seconds, "ms_per_update": 1e3 * seconds / weak_steps,
                "update_equivalents_per_s": weak_steps * world / seconds,
                "unit_definition": "update_equivalents = 2000-feature updates' worth of features per second",
                "steps": weak_steps, "exchange": "group triangles" if groups else "root blocks", "scaling": "weak"},
        })
    return line


if __name__ == "__main__":
    main()
