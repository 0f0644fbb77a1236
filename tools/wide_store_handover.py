#!/usr/bin/env python3
"""Batch hand-over of a frame on a wide-track context, through the track store and through the host door.

The run is the 40-clone run of tests/test_gpu_wide_store.py (`wide_store_cases.run_frames`: 45 frames, 12 tracks, tracks of
more than 32 views from frame 33 on, the nominal state resident, one prune-shaped removal at 40 clones).  Timed, as
`tools/frame_loop.py --loop c` times it for the narrow store: what it takes to put a frame's candidates -- every live track
-- in front of `run_select`, up to a stream sync.
  host   `UpdateEngine(max_track=64)`: `nominal()` (the bases live on the device after an injection), the bases resolved on
         the host (`cam_t[slot]`, the anchor or frozen base), `set_features`, `set_tracks`; the caller's track lists are kept,
         and flattened into the batch's arrays, outside the timed stretch
  store  `UpdateEngine(max_track=64, wide_store=True)`: `tracks_observe` + `load_tracks`
The selection, the update and the injection run on both sides and stay outside the timed stretch.  Both sides in one
process, interleaved run by run after one untimed run each.

    python tools/wide_store_handover.py [--runs 7] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import wide_store_cases as ws                        # noqa: E402
from msckf_amd import _ffi, synth                    # noqa: E402


def drive(eng, side):
    """One pass over the run; returns (the timed seconds of every frame, the views of the longest candidate per frame)."""
    K = synth.K_DEFAULT.copy()
    Kinv = np.linalg.inv(K)
    params = synth.SelectParams(**ws.PARAMS)
    clock = time.perf_counter
    tracks, out, longest = {}, [], []     # id -> dict(slots, uv, dir, conf, m, rho, anchor (slot or -1), frozen, lost, tracked)
    for f, nom, seen, px, score in ws.run_frames(eng):
        N = eng.n_clones
        R = nom["cam_R"][-1]
        for t in tracks.values():
            t["lost"] += 1
        for k, i in enumerate(seen):      # the caller's own lists (both sides keep the counters; the host side keeps the floats too)
            d = R @ (Kinv @ np.append(px[k], 1.0))
            t = tracks.setdefault(i, dict(slots=[], uv=[], dir=[], conf=[], m=d / np.linalg.norm(d), rho=0.1, anchor=N - 1, frozen=None, lost=0, tracked=0))
            t["slots"].append(N - 1); t["uv"].append(px[k]); t["dir"].append(d); t["conf"].append(score[k])
            t["lost"], t["tracked"] = 0, t["tracked"] + 1
        ids = list(tracks)
        lost = np.array([tracks[i]["lost"] for i in ids], np.int32)
        tracked = np.array([tracks[i]["tracked"] for i in ids], np.int32)
        if side == "host":                # the caller's batch arrays, ready before the clock starts: all but the bases
            slot = np.concatenate([tracks[i]["slots"] for i in ids]).astype(np.int32)
            anchor = np.array([tracks[i]["anchor"] for i in ids])
            frozen = np.array([tracks[i]["frozen"] if tracks[i]["frozen"] is not None else np.zeros(3) for i in ids]).reshape(-1, 3)
            b = dict(view_ptr=np.concatenate([[0], np.cumsum([len(tracks[i]["slots"]) for i in ids])]).astype(np.int32),
                     obs_uv=np.concatenate([tracks[i]["uv"] for i in ids]).reshape(-1, 2), obs_slot=slot,
                     line_dir=np.concatenate([tracks[i]["dir"] for i in ids]).reshape(-1, 3),
                     line_conf=np.concatenate([tracks[i]["conf"] for i in ids]),
                     idp_m=np.array([tracks[i]["m"] for i in ids]).reshape(-1, 3), idp_rho=np.array([tracks[i]["rho"] for i in ids]))
            state = (np.zeros((15 + 6 * N,) * 2), np.zeros((N, 3, 3)), np.zeros((N, 3)))      # (set_features reads no state)
        eng.sync()
        t0 = clock()
        if side == "host":
            cam_t = eng.nominal()["cam_t"]
            b["line_base"] = cam_t[slot]
            b["idp_base"] = np.where((anchor >= 0)[:, None], cam_t[np.maximum(anchor, 0)], frozen)
            eng.set_features(ws.problem_of(b, *state, synth.GRAVITY_DEFAULT, K, ws.RUN_SIGMA))
            eng.set_tracks(ws.tracks_of(b, lost, tracked))
        else:
            eng.tracks_observe(seen, px, score)
            eng.load_tracks(ids, lost, tracked)
        eng.sync()
        out.append(clock() - t0)
        longest.append(max(len(tracks[i]["slots"]) for i in ids))
        eng.run_select(params, K)
        sel = eng.selection()
        for k, i in enumerate(ids):
            if sel.flags[k] & _ffi.SEL_REFRESHED:
                tracks[i]["m"], tracks[i]["rho"] = sel.idp_m[k].copy(), float(sel.idp_rho[k])
        if int(sel.valid.sum()):
            eng.run()
            eng.result()
            eng.commit_inject()
        gone = [i for k, i in enumerate(ids) if sel.flags[k] & _ffi.SEL_LOST]
        if side == "store" and gone:
            eng.tracks_remove(gone)
        for i in gone:
            del tracks[i]
        if f == ws.RUN_PRUNE_AT:
            before = eng.nominal()["cam_t"]
            keep = [s for s in range(N) if s not in ws.RUN_PRUNE]
            remap = {s: k for k, s in enumerate(keep)}
            eng.remove_clones(ws.RUN_PRUNE)
            for i, t in list(tracks.items()):
                sel_v = [k for k, s in enumerate(t["slots"]) if s in remap]
                for name in ("uv", "dir", "conf"):
                    t[name] = [t[name][k] for k in sel_v]
                t["slots"] = [remap[t["slots"][k]] for k in sel_v]
                if t["anchor"] >= 0 and t["anchor"] not in remap:
                    t["frozen"], t["anchor"] = before[t["anchor"]].copy(), -1
                elif t["anchor"] >= 0:
                    t["anchor"] = remap[t["anchor"]]
                if not t["slots"]:
                    del tracks[i]
    return out, longest


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    sides = ["host", "store"]
    engines = {"host": ws.door_engine(max_clones=42), "store": ws.wide_engine(max_clones=42)}
    per_run = {sd: [] for sd in sides}
    for sd in sides:
        _, longest = drive(engines[sd], sd)                       # warm-up
    for _ in range(args.runs):
        for sd in sides:
            per_run[sd].append(drive(engines[sd], sd)[0])
    wide = np.array(longest) > 32
    lines = [f"batch hand-over of a frame on a wide-track context, {len(longest)} frames of at most {len(ws.RUN_TRACKS)} tracks, "
             f"{int(wide.sum())} of them with a track of more than 32 views (longest {max(longest)}), {args.runs} runs; us per frame, median (min .. max of the runs' medians)"]
    names = {"host": "nominal() + host bases + set_features + set_tracks", "store": "tracks_observe + load_tracks"}
    for what, pick in (("every frame", np.ones(len(longest), bool)), ("frames with a wide track", wide)):
        lines.append(f"  {what}")
        med = {}
        for sd in sides:
            t = np.array(per_run[sd])[:, pick] * 1e6
            meds = np.median(t, axis=1)
            med[sd] = np.median(meds)
            lines.append(f"    {names[sd]:52s} {np.median(t):8.1f} ({meds.min():.1f} .. {meds.max():.1f})   p10 {np.percentile(t, 10):8.1f}   p90 {np.percentile(t, 90):8.1f}")
        lines.append(f"    host / store of the runs' medians: {med['host'] / med['store']:.2f}x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
