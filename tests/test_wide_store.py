"""The track store of a wide-track context (`MSCKF_FLAG_WIDE_STORE`, `UpdateEngine(..., wide_store=True)`), the CPU side:
the flag's value in the header and in Python, the constructor's refusal, the host mirror at rows of 64 views against
`track_mirror_model.py`, and the conditions the cases of tests/test_gpu_wide_store.py have to meet (tests/wide_store_cases.py),
decided from `oracle.associate`, `oracle.select_features`, `oracle.update` and the match restatements alone."""
import inspect
import os
import re

import numpy as np
import pytest

import test_track_mirror as tm
import wide_cases
import wide_store_cases as ws
from conftest import ROOT
from track_mirror_model import ERR_ARG

driver = tm.driver                # the fixture that builds tests/track_mirror_driver.cpp from csrc/track_mirror.h


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_flag_value_in_the_header_and_in_python():
    from msckf_amd import _ffi
    with open(os.path.join(ROOT, "include", "msckf_mi355x.h")) as f:
        hdr = f.read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MSCKF_FLAG_\w+) (\d+)", hdr)}
    assert vals["MSCKF_FLAG_WIDE_STORE"] == _ffi.FLAG_WIDE_STORE == 4
    assert vals["MSCKF_FLAG_TREE_PLAN"] == 1 and vals["MSCKF_FLAG_BAND_ONLY"] == 2       # (the bits do not overlap)
    assert _ffi.MAX_TRACK_ROW == 32 and _ffi.MAX_TRACK_WIDE == 64


def test_the_constructor_takes_wide_store():
    from msckf_amd.api import UpdateEngine
    par = inspect.signature(UpdateEngine.__init__).parameters
    assert "wide_store" in par and par["wide_store"].default is False


def test_f32_with_wide_rows_is_refused_before_any_library_call(monkeypatch):
    from msckf_amd import _ffi
    from msckf_amd.api import UpdateEngine

    def no_load():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_ffi, "load", no_load)
    with pytest.raises(ValueError):
        UpdateEngine(max_clones=40, max_features=8, max_track=33, dtype="f32", wide_store=True)
    with pytest.raises(ValueError):
        UpdateEngine(max_clones=40, max_features=8, max_track=64, dtype="f32", wide_store=True)
    with pytest.raises(AssertionError):                        # 32 views: nothing to refuse, the call goes on to the library
        UpdateEngine(max_clones=40, max_features=8, max_track=32, dtype="f32", wide_store=True)


# ---- the mirror at rows of 64 views ---------------------------------------------------------------------------------------
def test_mirror_rows_of_64_views(driver):
    """Rows growing to 64 views, the full-row refusal at the 65th, clone removals that empty a row, creation order."""
    T, V = 4, 64
    script = [tm.words("size", T, V)]
    for s in range(64):                                         # 7 in every clone; 3 in clones 0..31; 9 from clone 32 on
        ids = [7] + ([3] if s < 32 else [9])
        script.append(tm.words("observe", s, len(ids), *ids))
    full_at = len(script)
    script.append(tm.words("observe", 64, 2, 9, 7))             # a 65th clone: 7 is full, the first offender is pair 1
    script.append(tm.words("observe", 64, 1, 9))                # 9 alone goes in: 33 views
    script.append("created")
    script.append(tm.words("frame", 64, 0, 2, 5, 1, 4, 7, 1, 0))     # ... and a frame that lists 7 is refused the same way
    refused_frame = len(script) - 1
    script.append(tm.words("drop", 65, *[int(s < 32) for s in range(65)]))       # clones 0..31 go: 3 is emptied, 7 keeps 32 views
    dropped_at = len(script) - 1
    script.append(tm.words("observe", 32, 2, 7, 5))             # 33 clones left, the newest is slot 32; 5 takes 3's row
    script.append("created")
    blocks = driver("wide_rows", script)
    m = tm.replay(script, blocks)
    assert all(b[0] == "rc 0 bad -1" for b in blocks[:full_at])
    assert any(line.startswith("id 7 ") and len(line.split("slots")[1].split()) == 64 for line in blocks[full_at - 1])
    assert blocks[full_at][0] == "rc %d bad 1" % ERR_ARG and tm.state(blocks[full_at]) == tm.state(blocks[full_at - 1])
    assert blocks[refused_frame][0] == "rc %d bad 1" % ERR_ARG and tm.state(blocks[refused_frame]) == tm.state(blocks[refused_frame - 1])
    assert tm.state(blocks[dropped_at])[0].endswith("dropped 3")
    assert m.ids_created_order() == [7, 9, 5]
    assert m.live[7]["slots"] == list(range(33)) and m.live[7]["anchor"] == -1 and m.live[9]["anchor"] == 0
    assert m.live[5]["row"] == 1                                # the row 3 left


# ---- the GPU cases ----------------------------------------------------------------------------------------------------------
def test_frame_cases_place_their_failures_where_the_kernel_can_go_wrong():
    c = ws.frame_case()
    res, fail = c["res"], c["fail"]
    want = [(k if k is not None else -1, kind) for _, _, k, kind in ws.FRAME_TRACKS]
    print("frame intake: results", res.tolist(), "first failing views", fail.tolist())
    print(f"frame intake: largest honest score / threshold {c['honest']:.3f}, smallest displaced one {c['displaced']:.1f}")
    assert [(int(f), int(r)) for r, f in zip(res, fail)] == want
    assert {0, 31, 32} <= set(fail.tolist()) and (fail >= 33).any()
    assert ((res == 1) & (fail >= 32)).any() and ((res == 2) & (fail >= 32)).any()
    for i, (k2, kind2) in ws.FRAME_LATER.items():               # two failures, one on either side of bit 32: the first decides
        j = c["ids"].index(i)
        k1, kind1 = ws.FRAME_TRACKS[j][2:]
        assert (k1 < 32 <= k2 or 32 <= k1 < k2) and kind1 != kind2 and len(c["views"][j]) == 63
        assert (int(fail[j]), int(res[j])) == (k1, kind1)
    assert any(k1 < 32 <= ws.FRAME_LATER[i][0] for i, _, k1, _ in ws.FRAME_TRACKS if i in ws.FRAME_LATER)
    rows = sorted({len(v) for v in c["views"]})
    assert rows == [1, 31, 32, 33, 63]
    for n in rows:                                              # on every row length a pair passes and a pair fails
        kinds = {int(r) > 0 for r, v in zip(res, c["views"]) if len(v) == n}
        assert kinds == {False, True}, n
    assert c["honest"] * ws.FRAME_SEPARATION <= 1.0 and c["displaced"] >= ws.FRAME_SEPARATION
    assert len(c["ids"]) + 1 <= 16 and ws.FRAME_FULL in c["ids"] and len(c["views"][c["ids"].index(ws.FRAME_FULL)]) == 63


@pytest.mark.parametrize("name", sorted(ws.UPDATE_CASES))
def test_no_update_case_sits_on_a_gate_threshold(name):
    c = ws.update_case(name)
    nv = [len(v) for v in c["views"]]
    m = wide_cases.margin(c["ref"])
    print(f"{name}: views {nv}, valid {c['valid'].tolist()}, accepted {c['ref']['accepted'].tolist()}, gate margin {m:.4f}")
    assert m >= wide_cases.MIN_MARGIN
    assert c["ref"]["status"] == 0 and c["ref"]["accepted"].any()
    assert [n for n in nv if n > 1] == [nv[j] for j in c["valid"]]           # every track of two views and more is a candidate
    assert (c["sel"]["flags"][c["valid"]] & 4).all()                         # ... and its point was refreshed
    if name == "w48":
        assert {31, 32, 33, 48, 1, 2, 10} <= set(nv) and any(np.any(np.diff(v) > 1) for v in c["views"])
    else:
        assert {63, 64, 1, 2, 10} <= set(nv) and list(range(32, 64)) in c["views"]


@pytest.mark.parametrize("mode", sorted(ws.MATCH_MODES))
def test_descriptor_walks_keep_their_similarities_off_the_thresholds(mode):
    """The restatement runs with its guards on: it raises where a similarity, a runner-up, a margin or a distance is near
    its threshold, and where the reference would skip a frame."""
    c = ws.match_case()
    radius, margin = ws.MATCH_MODES[mode]
    st, log = ws.walk_model(c["p"], c["frames"], radius, margin)
    assert None not in log                                      # no frame is skipped
    nv = sorted(len(t.uv) for t in st.tracks.values())
    print(f"{mode}: views per track {nv}")
    assert len(st.tracks) == len(c["views"]) and nv == sorted(len(v) for v in c["views"])       # no track was torn
    assert set(range(33, 41)) <= set(nv)
    if radius:
        assert any(e[2] is not None and (e[2] == 1).any() for e in log)        # a track with no keypoint inside its window


def test_drop_walks_meet_the_guards_and_the_sets_are_the_ones_that_count():
    c = ws.drop_case()
    st, log = ws.walk_model(c["p"], c["frames"])
    assert None not in log
    assert sorted(len(t.uv) for t in st.tracks.values()) == sorted(len(v) for v in c["views"]) and len(c["views"][0]) == 64
    assert ws.DROP_SETS["the_four_corners"] == [0, 31, 32, 63] and ws.DROP_SETS["lower_half_and_the_anchor"] == list(range(32))
    c = ws.drop100_case()
    st, _ = ws.walk_model(c["p"], c["frames"])
    assert c["views"][0] == list(range(36, 100)) and [c["views"][0].index(s) for s in ws.DROP100_SET] == [0, 31, 32, 63]
    assert max(len(t.uv) for t in st.tracks.values()) == 64 and len(st.tracks) == 3      # (frames without a keypoint are not sent)
