"""Per-frame intake time from descriptors on the resident engine, the twelve frames of
`tests/golden/match/match_frames.npz`:

  device  `tracks_match_frame` (match on the device + tests + append + counters + rows, one blocking call)
  host    the route without it: the host keeps every track's descriptors and the table, runs the NumPy
          mutual-nearest-neighbour match, numbers the new tracks and calls `tracks_frame`

Both drive the whole run (clones, removals, the prune) and time only the intake of each frame: wall time around the
calls, the stream drained before and after.  The first run of each route is a warm-up; the routes are interleaved; the
figure is the median over frames of the per-frame medians over the runs.  A record, not a gate.

    python tools/match_intake.py [--runs 9] [--radius inf] [--margin 0]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import frame_cases          # noqa: E402
import match_ref            # noqa: E402


def drive(fx, eng, route):
    z = fx.z
    min_cos, thr_e, thr_h = (float(x) for x in z["params"])
    eng.set_prior(np.eye(15) * 0.01, np.array([0.0, 0.0, -9.81]), z["K"], 1.0)
    keys, last_id, times = [], 0, []
    desc, score, table_ids, table = {}, {}, [], None                 # the host route's copy of what the store keeps
    for f in range(fx.n_frames):
        fr = fx.frame(f)
        eng.augment(frame_cases.J15, fr["R"], fr["t"])
        keys.append(int(fr["key"]))
        eng.sync()
        t0 = time.perf_counter()
        if route == "device":
            eng.tracks_match_frame(fr["kp"], fr["desc"], fr["score"], z["K"], last_id + 1, min_cos, thr_e, thr_h)
        else:
            n = len(fr["kp"])
            ids = np.full(n, -1, dtype=np.int32)
            go = True
            if table_ids:
                idx1, idx2, _ = match_ref.match(table, fr["desc"], min_cos)
                ids[idx2] = np.asarray(table_ids)[idx1]
                go = len(idx1) > 0
            if go:
                new = ids < 0
                ids[new] = last_id + 1 + np.arange(int(new.sum()))
                res, _ = eng.tracks_frame(ids, fr["kp"], fr["score"], z["K"], thr_e, thr_h)
                for j in np.nonzero((res == 0) | (res == 4))[0]:
                    desc.setdefault(int(ids[j]), []).append(fr["desc"][j])
                    score.setdefault(int(ids[j]), []).append(fr["score"][j])
                table_ids = list(desc)
                table = np.array([np.average(np.asarray(desc[i], dtype=np.float64), axis=0, weights=score[i]) for i in table_ids],
                                 dtype=np.float32)
        eng.sync()
        times.append(time.perf_counter() - t0)
        last_id = int(fr["last_id"])
        # the frame's removals, as tests/test_gpu_tracks_match.py applies them (untimed)
        gone = set(fr["rm_tracks"].tolist())
        if gone:
            eng.tracks_remove(fr["rm_tracks"])
        rm = [keys.index(int(c)) for c in fr["rm_keys"] if int(c) in keys]
        if rm and len(rm) < len(keys):
            views = {i: eng.track(i)["slots"].tolist() for i in desc if i not in gone} if route == "host" else {}
            eng.remove_clones(rm)
            keys = [c for s, c in enumerate(keys) if s not in rm]
            gone |= set(eng.tracks_dropped().tolist())
            for i, sl in views.items():
                keep = [v for v, s in enumerate(sl) if s not in rm]
                desc[i], score[i] = [desc[i][v] for v in keep], [score[i][v] for v in keep]
        if route == "host" and gone:
            keep = [k for k, i in enumerate(table_ids) if i not in gone]
            table_ids, table = [table_ids[k] for k in keep], table[keep]
            for i in gone:
                desc.pop(i, None), score.pop(i, None)
    eng.tracks_reset()
    return np.array(times) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--radius", type=float, default=None, help="search_radius of set_match_options on the device route (inf is legal)")
    ap.add_argument("--margin", type=float, default=None, help="min_margin of set_match_options on the device route")
    a = ap.parse_args()
    from msckf_amd.api import UpdateEngine
    fx = match_ref.Fixture()
    out = {}
    for route in ("host", "device", "host", "device"):              # interleaved: two blocks of `runs` each
        out.setdefault(route, [])
        for _ in range(a.runs + 1):
            with UpdateEngine(max_clones=16, max_features=512, max_track=32) as eng:
                if route == "device" and (a.radius is not None or a.margin is not None):
                    eng.set_match_options(a.radius, a.margin)           # (a finite radius changes the pairs, and with them the run)
                t = drive(fx, eng, route)
            out[route].append(t)
        del out[route][-(a.runs + 1)]                                # each block's first run is a warm-up
    n = np.mean([len(fx.frame(f)["kp"]) for f in range(fx.n_frames)])
    for route, t in out.items():
        t = np.array(t)
        per_frame = np.median(t, axis=0)
        meds = np.median(t, axis=1)
        print(f"{route:6s} intake per frame: {np.median(per_frame):7.1f} us (runs' medians {meds.min():.1f} - {meds.max():.1f}; "
              f"{t.shape[1]} frames, {t.shape[0]} runs, mean keypoints {n:.0f}, D = {int(fx.z['desc_dim'])})")


if __name__ == "__main__":
    main()
