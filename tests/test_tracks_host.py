"""CPU checks behind the resident track store (`msckf_tracks_*`).

(a) The event stream `track_events.py` derives from the 30-clone fixture is sound: replayed in plain Python it rebuilds,
    at every one of the 53 calls, each candidate's view list (the call's `pool` slice), the live set at `PROCESS` calls
    (`call_ids`) and the tracks that leave each call (`exit_ids` / `exit_nview`).
(b) Every stored line direction is `R_aug K^-1 [u, v, 1]` bit for bit (`Camera.py:30-44`), with the pose the clone was
    augmented with: what `tracks_observe` forms on the device.
(c) The header declares the new entry points and `_ffi` binds them with the documented argument types."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import track_events
import window30
from conftest import ROOT
from window30 import PROCESS, PRUNE, REMOVE

NAMES = ["msckf_tracks_reset", "msckf_tracks_observe", "msckf_tracks_remove", "msckf_tracks_load", "msckf_tracks_get",
         "msckf_tracks_count", "msckf_tracks_dropped"]


@pytest.fixture(scope="module")
def run():
    return window30.Run()


def test_event_stream_replays_every_call(run):
    events = track_events.derive(run)
    assert len(events) == run.n_calls() == 53
    got = track_events.replay(run, events)
    assert got == dict(created=468, appended=len(run.z["pool_uv"]), alive=119) and got["appended"] == 4468, got
    assert REMOVE not in [k for k, _ in run.ops]
    # observations arrive at PROCESS calls only; prunes remove clones, and only they do in this run
    for ev in events:
        assert (ev["kind"] == PROCESS) or len(ev["observe_ids"]) == 0
        assert (ev["kind"] == PRUNE) == (len(ev["rm"]) > 0)
    # (no prune of this run leaves a track without a view: that path is test_gpu_tracks.py's hand-built case)
    assert sum(len(ev["remove"]) for ev in events) > 0 and sum(len(ev["dropped"]) for ev in events) == 0


def test_pool_directions_are_the_augmentation_pose_times_the_back_projection(run):
    z = run.z
    Kinv = np.linalg.inv(z["K"])                                        # Camera.py:35
    R_of = {int(k): R for k, R in zip(z["aug_key"], z["aug_cam_R"])}
    for uv, key, d in zip(z["pool_uv"].astype(np.float64), z["pool_key"], z["pool_dir"]):
        assert np.array_equal(R_of[int(key)] @ (Kinv @ np.append(uv, 1)), d)


def test_header_declares_and_ffi_binds_the_track_entry_points(engine_lib):
    from msckf_amd import _ffi
    txt = open(os.path.join(ROOT, "include", "msckf_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    vp, ip, dp = C.c_void_p, C.c_void_p, C.c_void_p
    want = {
        "msckf_tracks_reset": [vp],
        "msckf_tracks_observe": [vp, C.c_int32, ip, dp, dp],
        "msckf_tracks_remove": [vp, C.c_int32, ip],
        "msckf_tracks_load": [vp, C.c_int32, ip, ip, ip],
        "msckf_tracks_get": [vp, C.c_int32, ip, ip, dp, dp, dp, dp, dp, dp, dp, ip],
        "msckf_tracks_count": [vp, ip, ip],
        "msckf_tracks_dropped": [vp, ip, C.c_int32],
    }
    assert sorted(want) == sorted(NAMES)
    for name, argtypes in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _ffi.SYMBOLS, name
        fn = getattr(engine_lib, name)
        assert fn.argtypes == argtypes and fn.restype is C.c_int, name
    from msckf_amd.api import UpdateEngine
    for meth in ("tracks_reset", "tracks_observe", "tracks_remove", "load_tracks", "track", "tracks_count", "tracks_dropped"):
        assert callable(getattr(UpdateEngine, meth)), meth
    assert _ffi.ABI_VERSION == 2
