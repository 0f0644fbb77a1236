"""The 30-clone run (`golden/window30/seq_window30.npz`) as the front end's per-frame events: what a caller of the track
store (`tracks_observe` / `load_tracks` / `tracks_remove` / `remove_clones`) sends, derived from the stored calls.

Per selection call (`window30.Run.call`), in the order the caller acts:
  observe   PROCESS calls only: the views whose clone key is the window's newest (`MSCKF.add_camera_measurements` ran just
            before, `MSCKF.py:403-411`, `:420-434`) -- track ids, global pool indices; a track not alive yet is a creation
  cand      the candidates, in the call's order (`get_valid_features`' input)
  remove    after the update: tracks `remove_features` deletes (`:739-741`) -- alive, absent from the call's exit set and
            not merely left without a view by the clone removal
  rm        clone slots removed after the update (`remove_cameras`, `:751-779`)
  dropped   tracks that removal leaves without a view
Not a conftest: imported by name."""
import numpy as np

from window30 import PROCESS


def derive(run):
    """List of per-call event dicts; keeps a {id: [pool index]} replay to tell `remove` from `dropped`."""
    z = run.z
    live, out = {}, []
    for i in range(run.n_calls()):
        c = run.call(i)
        vp, ids = c["view_ptr"], c["ids"].tolist()
        ob_ids, ob_pool = [], []
        if c["kind"] == PROCESS:
            newest = int(c["keys"][-1])
            for j, fid in enumerate(ids):
                last = int(c["pool"][vp[j + 1] - 1])
                if int(z["pool_key"][last]) == newest:
                    ob_ids.append(fid)
                    ob_pool.append(last)
                    live.setdefault(fid, []).append(last)
        rm_keys = {int(c["keys"][s]) for s in c["rm"]}
        exit_ids = set(c["exit_ids"].tolist())
        after = {fid: [p for p in views if int(z["pool_key"][p]) not in rm_keys] for fid, views in live.items()}
        dropped = [fid for fid, views in after.items() if not views]
        remove = [fid for fid, views in after.items() if views and fid not in exit_ids]
        live = {fid: views for fid, views in after.items() if views and fid in exit_ids}
        out.append(dict(call=i, kind=c["kind"], observe_ids=np.array(ob_ids, dtype=np.int32), observe_pool=np.array(ob_pool, dtype=np.int64),
                        cand=c["ids"].astype(np.int32), remove=np.array(remove, dtype=np.int32), rm=c["rm"].astype(np.int32),
                        dropped=sorted(dropped)))
    return out


def replay(run, events):
    """The events alone rebuild every call's candidates, live set and exit set.  Returns counters."""
    z = run.z
    live = {}
    created = appended = 0
    for ev in events:
        c = run.call(ev["call"])
        for fid, p in zip(ev["observe_ids"].tolist(), ev["observe_pool"].tolist()):
            created += int(fid not in live)
            live.setdefault(fid, []).append(p)
            appended += 1
        vp = c["view_ptr"]
        for j, fid in enumerate(ev["cand"].tolist()):
            assert live[fid] == c["pool"][vp[j]:vp[j + 1]].tolist(), (ev["call"], fid)
        if c["kind"] == PROCESS:
            assert list(live) == c["ids"].tolist(), ev["call"]
        for fid in ev["remove"].tolist():
            del live[fid]
        rm_keys = {int(c["keys"][s]) for s in ev["rm"]}
        dropped = []
        for fid in list(live):
            live[fid] = [p for p in live[fid] if int(z["pool_key"][p]) not in rm_keys]
            if not live[fid]:
                dropped.append(fid)
                del live[fid]
        assert sorted(dropped) == ev["dropped"], ev["call"]
        assert {fid: len(v) for fid, v in live.items()} == dict(zip(c["exit_ids"].tolist(), c["exit_nview"].tolist())), ev["call"]
    return dict(created=created, appended=appended, alive=len(live))
