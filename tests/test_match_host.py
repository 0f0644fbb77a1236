"""Frame intake from descriptors, the host side: the restatement in `match_ref.py` against what the reference itself did
with the fixture's frames (`golden/match/match_frames.npz`, `golden/gen_match_golden.py`), the guards that make those
frames a fair test of a matcher that rounds its sums differently, and the C-ABI's declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import match_ref


@pytest.fixture(scope="module")
def fx():
    return match_ref.Fixture()


def _ulp_ok(got32, ref64):
    """Within one fp32 ulp of the reference's fp64 value."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return np.all(np.abs(np.asarray(got32, dtype=np.float64) - ref64) <= np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64))


def _check_state(fx, store, fr, stage, f):
    want = fx.tracks(fr, stage)
    assert list(store.tracks) == list(want), (f, stage)
    for tid, tr in store.tracks.items():
        assert (tr.keys, tr.lost, tr.tracked) == want[tid], (f, stage, tid)
    got_desc = np.array([d for tr in store.tracks.values() for d in tr.desc], dtype=np.float32).reshape(-1, fr["desc"].shape[1])
    assert np.array_equal(got_desc.view(np.uint32), fr[stage + "_desc"].view(np.uint32)), (f, stage)
    assert store.table_ids == fr[stage + "_table_ids"].tolist(), (f, stage)
    assert _ulp_ok(store.table, fr[stage + "_table"]), (f, stage)


def test_the_restatement_reproduces_the_reference_frame_by_frame(fx):
    z = fx.z
    min_cos, thr_e, thr_h = z["params"]
    store = match_ref.Store(z["K"], min_cos, thr_e, thr_h)
    seen = dict(skipped=0, raw=0, stale=0, codes=set())
    for f in range(fx.n_frames):
        fr = fx.frame(f)
        store.add_camera(int(fr["key"]), fr["R"], fr["t"])
        raw = not store.tracks
        out = store.intake(int(fr["key"]), fr["kp"], fr["desc"], fr["score"])
        assert (out is None) == bool(fr["skipped"]), f
        if out is None:
            seen["skipped"] += 1
        else:
            ids, res, pairs = out
            assert np.array_equal(ids, fr["ids"]) and np.array_equal(res, fr["result"]) and np.array_equal(pairs, fr["pairs"]), f
            seen["codes"] |= set(res.tolist())
            if raw:
                seen["raw"] += 1
                assert np.array_equal(store.table.view(np.uint32), fr["desc"].view(np.uint32))
        assert store.last_id == int(fr["last_id"])
        _check_state(fx, store, fr, "in", f)
        store.remove_tracks(fr["rm_tracks"].tolist())
        dropped = store.remove_cameras(fr["rm_keys"].tolist())
        assert sorted(dropped) == fr["dropped"].tolist(), f
        if len(fr["rm_keys"]) and store.tracks and not len(fr["rm_tracks"]):
            # a prune: some track lost a view and its row did not move
            k = {t: i for i, t in enumerate(fr["in_table_ids"].tolist())}
            stale = [t for t in store.tracks if len(store.tracks[t].keys) < np.diff(fr["in_ptr"])[k[t]]]
            assert stale and all(np.array_equal(store.table[store.table_ids.index(t)], fr["in_table"][k[t]].astype(np.float32)) or
                                 _ulp_ok(store.table[store.table_ids.index(t)], fr["in_table"][k[t]]) for t in stale)
            seen["stale"] += 1
        _check_state(fx, store, fr, "out", f)
    # the run has what the issue asks of it: a skipped frame, a prune between frames, two frames on an empty store
    assert seen["skipped"] == 1 and seen["stale"] == 1 and seen["raw"] == 2 and seen["codes"] == {0, 1, 2, 4}, seen


def test_the_guards_hold_on_every_frame_that_meets_a_table(fx):
    z = fx.z
    min_cos = float(z["params"][0])
    checked = 0
    for f in range(1, fx.n_frames):
        prev, fr = fx.frame(f - 1), fx.frame(f)
        A = prev["out_table"]
        assert fr["desc"].dtype == np.float32 and fr["desc"].shape[1] == 8 and len(fr["desc"]) <= 60
        if len(A) == 0:
            continue
        g = match_ref.guards(A, fr["desc"], min_cos, need_pairs=not bool(fr["skipped"]))
        assert (g["pairs"] == 0) == bool(fr["skipped"])
        if not fr["skipped"]:
            assert g["pairs"] == len(fr["pairs"])
        checked += 1
    assert checked >= 9


def test_match_rule_ties_go_to_the_lowest_index():
    A = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], dtype=np.float32)
    B = np.array([[0.0, 2.0], [3.0, 0.0], [3.0, 0.0]], dtype=np.float32)
    idx1, idx2, S = match_ref.match(A, B, 0.5)
    assert idx1.tolist() == [0, 2] and idx2.tolist() == [1, 0] and S[0, 1] == 3.0
    assert match_ref.match(A, B, 3.0)[0].tolist() == []             # the comparison is strict


def _header():
    txt = open(os.path.join(ROOT, "include", "msckf_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_three_calls_and_ffi_binds_them(engine_lib):
    from msckf_amd import _ffi
    txt = re.sub(r"\s+([,)])", r"\1", re.sub(r"\s+", " ", _header()))
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    want = {
        "msckf_tracks_match": (r"msckf_ctx\*\s*ctx,\s*double\s+\w+,\s*int32_t\s+\w+,\s*int32_t\s+n,\s*const float\*\s*desc,\s*int32_t\*\s*track_id_out,\s*float\*\s*sim_out",
                               [vp, f64, i32, i32, vp, vp, vp]),
        "msckf_tracks_match_frame": (r"msckf_ctx\*\s*ctx,\s*const msckf_match_params\*\s*params,\s*int32_t\s+n,\s*const float\*\s*desc,\s*const double\*\s*uv,"
                                     r"\s*const double\*\s*score,\s*int32_t\*\s*ids_out,\s*uint8_t\*\s*result,\s*int32_t\*\s*fail_view,\s*float\*\s*sim_out",
                                     [vp, C.POINTER(_ffi.MatchParamsC), i32, vp, vp, vp, vp, vp, vp, vp]),
        "msckf_tracks_descriptor": (r"msckf_ctx\*\s*ctx,\s*int32_t\s+id,\s*float\*\s*row,\s*int32_t\*\s*M,\s*float\*\s*views", [vp, i32, vp, vp, vp]),
    }
    for name, (proto, argtypes) in want.items():
        assert re.search(r"\bint\s+" + name + r"\(\s*" + proto + r"\s*\)\s*;", txt), name
        assert name in _ffi.SYMBOLS
        fn = getattr(engine_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name


def test_match_params_size_and_layout_match_the_header():
    from msckf_amd import _ffi
    body = re.search(r"typedef struct msckf_match_params\s*\{(.*?)\}\s*msckf_match_params;", _header(), flags=re.S).group(1)
    fields, off = [], 0
    for typ, name, dim in re.findall(r"(double|int32_t)\s+(\w+)(?:\[(\d+)\])?;", body):
        size = (8 if typ == "double" else 4)
        off = (off + size - 1) // size * size
        fields.append((name, off))
        off += size * int(dim or 1)
    size = (off + 7) // 8 * 8
    assert [n for n, _ in fields] == [n for n, _ in _ffi.MatchParamsC._fields_]
    assert all(getattr(_ffi.MatchParamsC, n).offset == o for n, o in fields)
    assert C.sizeof(_ffi.MatchParamsC) == size == 104
    # it begins as msckf_frame_params does
    assert [f[0] for f in _ffi.MatchParamsC._fields_[:3]] == [f[0] for f in _ffi.FrameParamsC._fields_]
