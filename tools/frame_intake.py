"""Per-frame intake time on the resident engine, the 30-clone reference run (`tests/golden/window30/seq_window30.npz`):

  store   `tracks_frame` (test + append + counters, one blocking call)
  host    the route without it: `nominal()` + `set_features` of the host's copy of the tracks + `associate` +
          `tracks_observe` of the matches that passed

Both drive the whole run (IMU batches, augmentation, selection, update, injection, removals) and time only the intake of
each `process_features` frame: wall time around the calls, the stream drained before and after.  The first run of each
route is a warm-up; the figure is the median over frames of the per-frame medians over the runs.

    python tools/frame_intake.py [--runs 5]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import nominal_ref          # noqa: E402
import track_events         # noqa: E402
import window30             # noqa: E402
from window30 import AUGMENT, PROCESS   # noqa: E402

INF = float("inf")


def drive(run, events, eng, route):
    from msckf_amd import synth
    z = run.z
    params = run.select_params()
    gyro, acc = nominal_ref.raw_samples(run)
    eng.set_prior(z["P0"], z["gravity"], z["K"], run.sigma)
    eng.set_nominal(z["imu_R0"][0], z["imu_t0"][0], z["imu_v0"][0], z["gravity"], z["Qc"],
                    T_W_I=(z["T_W_I_R"], z["T_W_I_t"]), T_W_C=(z["T_W_C_R"], z["T_W_C_t"]))
    times = []
    for kind, idx, o in nominal_ref.imu_groups(run):
        if kind == "imu":
            eng.propagate_imu(gyro[idx], acc[idx], z["imu_dt"][idx])
            continue
        if kind == AUGMENT:
            eng.augment_imu()
            continue
        c, ev = run.call(idx), events[idx]
        if kind == PROCESS:
            pool = ev["observe_pool"]
            ids, uv = ev["observe_ids"], z["pool_uv"][pool].astype(np.float64)
            score = z["pool_score"][pool].astype(np.float64)
            N = len(c["keys"])
            # the host's copy of the tracks as they stand before this frame's views (the candidates minus the newest clone's)
            vp, old = c["view_ptr"], c["obs_slot"] < N - 1
            nv = np.add.reduceat(old.astype(np.int64), vp[:-1]) if len(vp) > 1 else np.zeros(0, np.int64)
            has = nv > 0
            owner = np.repeat(np.arange(len(nv)), np.diff(vp))
            keep = old & has[owner]
            matched = np.full((int(has.sum()), 2), np.nan)
            row_of = {int(f): r for r, f in enumerate(c["ids"][has])}
            for f, p in zip(ids.tolist(), uv):
                if f in row_of:
                    matched[row_of[f]] = p
            eng.sync()
            t0 = time.perf_counter()
            if route == "store":
                eng.tracks_frame(ids, uv, score, z["K"], INF, INF)
            else:
                s = eng.nominal()
                if has.any():
                    prob = synth.UpdateProblem(P=None, cam_R=s["cam_R"], cam_t=s["cam_t"], cam_R0=s["cam_R"], cam_t0=s["cam_t"],
                                               gravity=z["gravity"], K=z["K"], sigma=run.sigma,
                                               view_ptr=np.concatenate([[0], np.cumsum(nv[has])]).astype(np.int32),
                                               obs_uv=c["obs_uv"][keep], obs_slot=c["obs_slot"][keep], idp_base=c["idp_base"][has],
                                               idp_m=c["idp_m"][has], idp_rho=c["idp_rho"][has])
                    eng.set_features(prob)
                    res, _ = eng.associate(matched, s["cam_R"][-1], s["cam_t"][-1], z["K"], INF, INF)
                    assert not ((res == 1) | (res == 2)).any()
                eng.tracks_observe(ids, uv, score)
                eng.sync()
            times.append(time.perf_counter() - t0)
        if route == "store":
            eng.load_tracks_where(None if kind == PROCESS else ev["rm"])
        else:
            eng.load_tracks(c["ids"], c["lost"], c["tracked"])
        eng.run_select(params, z["K"])
        sel = eng.selection()
        n_valid = int(sel.valid.sum())
        if 0 < n_valid < 0.15 * len(c["ids"]):
            eng.replan()
        if n_valid:
            eng.run()
            eng.commit_inject()
        eng.tracks_remove(ev["remove"])
        if len(ev["rm"]):
            eng.remove_clones(ev["rm"])
    return np.array(times) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    from msckf_amd.api import UpdateEngine
    run = window30.Run()
    events = track_events.derive(run)
    out = {}
    for route in ("host", "store", "host", "store"):                # interleaved: two blocks of `runs` each
        with UpdateEngine(max_clones=31, max_features=512, max_track=31) as eng:
            drive(run, events, eng, route)                           # warm-up
            out.setdefault(route, []).extend(drive(run, events, eng, route) for _ in range(a.runs))
    for route, t in out.items():
        t = np.array(t)
        per_frame = np.median(t, axis=0)
        meds = np.median(t, axis=1)
        print(f"{route:5s} intake per frame: {np.median(per_frame):7.1f} us (runs' medians {meds.min():.1f} - {meds.max():.1f}; "
              f"{t.shape[1]} frames, {t.shape[0]} runs, mean pairs {np.mean([len(e['observe_ids']) for e in events if e['kind'] == PROCESS]):.0f})")


if __name__ == "__main__":
    main()
