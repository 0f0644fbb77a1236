"""tests/wide_geometry_cases.py on the CPU: what every batch of tests/test_gpu_wide_coverage.py is FOR, recomputed from the batch,
and the conditions the oracle alone meets on it before the batch may run on the engine.

  lengths    `all_lengths` holds one track of every length 32 .. 64; the rank-2 batch reaches q = 2M - 2 = 64, 96, 112 (a full last
             strip of 16 rows) and 126; at 6M neither a multiple of 64 nor of 16 the masked tail of the gate's product loop decides
  layouts    holes, a first slot far from 0, a track wholly on slots of 128 and above, a track from slot 0 to slot N - 1, windows of
             65, 100 and 221 clones, an order that is neither ascending nor descending -- with oracle status 0, both gate verdicts
             among the wide tracks (N = 221: acceptance alone) and a gate margin of at least wide_cases.MIN_MARGIN
  geometry   the families at 32 .. 48 views under tests/test_geometry_cases.py's conditions; all six pivot orders of K2 on counted
             tracks and views with pz < 0 over the admitted cases

Seen (this file's prints, `-s`): in the tests' own docstrings."""
from collections import Counter

import numpy as np
import pytest

import geometry_cases as gc
import wide_cases as wc
import wide_geometry_cases as wg

_TABLES = {}


def table(name):
    if name not in _TABLES:
        _TABLES[name] = gc.track_table(wg.geometry(name)[0])
    return _TABLES[name]


def _verdicts(prob, ref):
    w, acc = wc.wide(prob), np.asarray(ref["accepted"]).astype(bool)
    return int((w & acc).sum()), int((w & ~acc).sum())


def _consecutive(prob):
    return all(np.array_equal(np.diff(wg.track_slots(prob, j)), np.ones(len(wg.track_slots(prob, j)) - 1)) for j in range(prob.F))


# ---- A ---------------------------------------------------------------------------------------------------------------------------

def test_all_lengths_holds_every_length():
    """Seen: 21 of the 33 tracks accepted, gate margin 0.115."""
    prob, ref = wg.all_lengths()
    M = wc.views(prob)
    assert prob.N == 64 and sorted(M.tolist()) == list(range(32, 65)) == list(wg.LENGTHS)
    assert _consecutive(prob)
    # what depends on M in k_feature_wide: the masked tail of the 64-deep product loop (6M no multiple of 64) and of the 16-column
    # chunks (6M no multiple of 16), the second Householder row of a lane (2M > 64), k_gather's second pass (M > 32)
    assert sum(6 * m % 64 != 0 for m in M) == 31 and sum(6 * m % 16 != 0 for m in M) >= 24
    q = 2 * M - 3
    assert {int(x) % 16 for x in q} == {1, 3, 5, 7, 9, 11, 13, 15} and len({(int(x) + 15) // 16 for x in q}) == 5
    acc, rej = _verdicts(prob, ref)
    m = wc.margin(ref)
    print(f"all_lengths: accepted {acc} rejected {rej} of {prob.F}, gate margin {m:.3e}")
    assert ref["status"] == 0 and acc >= 4 and rej >= 4 and m >= wc.MIN_MARGIN
    assert all(t[0].rank == 3 and t[0].margin >= gc.RANK_FACTOR for t in gc.track_table(prob))


def test_rank2_lengths_fill_whole_strips():
    """Seen: 15 of 21 accepted, gate margin 0.056, rank margin 51."""
    prob, ref = wg.all_lengths_rank2()
    M = wc.views(prob)
    assert prob.N == 64 and sorted(M.tolist()) == list(wg.RANK2_LENGTHS)
    assert set(range(32, 65, 2)) | {33, 63} <= set(M.tolist()) and _consecutive(prob)
    tab = gc.track_table(prob)
    for j, (qr, (rk, sm), _) in enumerate(tab):
        assert qr.rank == rk == 2 and qr.margin >= gc.RANK_FACTOR and sm >= gc.RANK_FACTOR, (j, qr.rank, rk, qr.margin, sm)
    q = set((2 * M - 2).tolist())
    assert {64, 96, 112, 126} <= q and wg.RANK2_FULL_STRIPS == {33: 64, 49: 96, 57: 112, 64: 126}
    from scipy.stats import chi2
    assert np.array_equal(ref["crit"], chi2.ppf(0.95, 2 * M - 2))
    acc, rej = _verdicts(prob, ref)
    m = wc.margin(ref)
    print(f"all_lengths_rank2: accepted {acc} rejected {rej} of {prob.F}, gate margin {m:.3e}, rank margin {min(t[0].margin for t in tab):.1f}")
    assert ref["status"] == 0 and acc >= 1 and rej >= 1 and m >= wc.MIN_MARGIN


# ---- B ---------------------------------------------------------------------------------------------------------------------------

def _holes(sl):
    s = np.sort(sl)
    return int(s[-1] - s[0] + 1 - len(s))


@pytest.mark.parametrize("name", ["holes_64", "shuffled", "beyond_65", "beyond_100", "beyond_221"])
def test_layout_batches_meet_the_oracles_conditions(name):
    """Seen (accepted / rejected wide tracks, gate margin): holes_64 and shuffled 6 / 1, 0.637; beyond_65 3 / 1, 0.450;
    beyond_100 2 / 2, 0.056; beyond_221 3 / 0, 0.731."""
    prob, ref = wg.layout_batches()[name]
    acc, rej = _verdicts(prob, ref)
    m = wc.margin(ref)
    print(f"{name}: N {prob.N} views {wc.views(prob).tolist()} wide accepted {acc} rejected {rej}, gate margin {m:.3e}")
    assert ref["status"] == 0 and m >= wc.MIN_MARGIN
    assert acc >= 1 and (rej >= 1 or prob.N == 221)
    assert all(len(set(wg.track_slots(prob, j).tolist())) == wc.views(prob)[j] for j in range(prob.F))
    assert prob.obs_slot.min() == 0 and prob.obs_slot.max() == prob.N - 1
    # what the engine does with it: no track is split (a batch with a wide track keeps one block per track)
    assert wc.views(prob).max() <= wg.WIDE_TO and (~wc.wide(prob)).sum() >= 2


def test_holes_64_layout():
    prob, _ = wg.holes_64()
    M, w = wc.views(prob), wc.wide(prob)
    assert prob.N == 64 and tuple(M[w]) == wg.HOLES_64_WIDE and tuple(M[~w]) == wg.HOLES_64_NARROW
    assert {32, 33, 40, 47, 63} <= set(M.tolist()) and {2, 10, 31} <= set(M.tolist())
    sl = [wg.track_slots(prob, j) for j in range(prob.F)]
    assert all(np.all(np.diff(s) > 0) for s in sl)                                    # ascending
    for j in range(5):                                                               # random subsets with holes
        assert _holes(sl[j]) >= 1 and sl[j][0] == 0 and sl[j][-1] == 63
    assert _holes(sl[0]) == 32 and np.any(np.diff(sl[0]) > 2)                       # (no regular pattern)
    assert np.array_equal(sl[5], np.arange(0, 64, 2)) and np.array_equal(sl[6], np.arange(32, 64))
    assert sum(_holes(s) > 0 for j, s in enumerate(sl) if not w[j]) >= 2            # narrow tracks with holes among them
    # a slot map that assumed slot = first slot + view is wrong on six of the seven wide tracks
    assert sum(not np.array_equal(s, s[0] + np.arange(len(s))) for j, s in enumerate(sl) if w[j]) == 6


def test_shuffled_order():
    prob, ref = wg.shuffled()
    base, base_ref = wg.holes_64()
    which = wg.shuffled_tracks(base)
    assert len(which) == 4 and wc.wide(base)[which].all()
    for j in range(prob.F):
        a, b = wg.track_slots(prob, j), wg.track_slots(base, j)
        if j in which:
            d = np.diff(a)
            assert sorted(a.tolist()) == b.tolist() and (d > 0).sum() >= 8 and (d < 0).sum() >= 8        # neither ascending nor reversed
        else:
            assert np.array_equal(a, b)
    # k_gather: the lowest slot of a track may sit among its views 32 and up, where only `min(sl, sl2)` sees it
    assert all(int(np.argmin(wg.track_slots(prob, j))) >= 32 for j in which if wc.views(prob)[j] > 32)
    assert sum(wc.views(prob)[j] > 32 for j in which) >= 2
    # k_feature_wide's gate: the first view is not on the lowest slot
    assert all(wg.track_slots(prob, j)[0] != wg.track_slots(prob, j).min() for j in which)
    # the pixels went with their slots
    for j in which:
        a, b = int(prob.view_ptr[j]), int(prob.view_ptr[j + 1])
        o = np.argsort(prob.obs_slot[a:b])
        assert np.array_equal(prob.obs_uv[a:b][o], base.obs_uv[a:b])
    # the oracle does not depend on the order, up to rounding
    assert np.array_equal(ref["accepted"], base_ref["accepted"])
    e = max(fb_rel(ref["dx"], base_ref["dx"]), fb_rel(ref["P_new"], base_ref["P_new"]), float(np.max(np.abs(ref["gamma"] / base_ref["gamma"] - 1.0))))
    print(f"shuffled against holes_64, the oracle's own spread: {e:.2e}")
    assert e < 1e-10


def fb_rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@pytest.mark.parametrize("N", list(wg.BEYOND))
def test_beyond_64_layout(N):
    prob, _ = wg.beyond_64(N)
    M, w = wc.views(prob), wc.wide(prob)
    sl = [wg.track_slots(prob, j) for j in range(prob.F)]
    assert prob.N == N > 64 and prob.d == 15 + 6 * N
    assert all(np.all(np.diff(s) > 0) for s in sl)
    wide_lengths = sorted(M[w].tolist())
    assert wide_lengths == ([32, 48, 64] if N == 221 else [32, 33, 48, 64])
    assert 2 <= int((~w).sum()) <= 3
    assert all(_holes(s) > 0 for j, s in enumerate(sl) if w[j])                      # every wide track skips clones
    assert any(w[j] and s[0] == 0 and s[-1] == N - 1 for j, s in enumerate(sl))     # slot 0 to slot N - 1
    assert any(w[j] and s.max() >= 64 for j, s in enumerate(sl))                     # slot numbers of 64 and above
    hs = wg.HIGH_SLOT[N]
    assert hs == (128 if N - 128 >= 32 else 64 if N - 64 >= 32 else None)           # the highest of 128, 64 the window has room above
    if hs is not None:
        assert any(w[j] and s.min() >= hs for j, s in enumerate(sl)), N
    if N == 221:
        assert any(w[j] and s.min() >= 128 for j, s in enumerate(sl))


def test_refused_batches_are_what_they_claim():
    for N, (prob, _) in ((64, wg.holes_64()), (65, wg.beyond_64(65))):
        j = int(np.argmax(wc.views(prob)))
        M = int(wc.views(prob)[j])
        dup = wg.with_duplicate_slot(prob, j, 3, M - 2)
        s = wg.track_slots(dup, j)
        assert prob.N == N and M - 2 >= 32 and len(set(s.tolist())) == M - 1 and s[M - 2] == s[3]
        assert np.array_equal(np.delete(s, M - 2), np.delete(wg.track_slots(prob, j), M - 2))
    prob, _ = wg.beyond_64(65)
    bad = wg.with_slot(prob, 0, 40, 65)
    assert bad.obs_slot.max() == prob.N == 65


# ---- C ---------------------------------------------------------------------------------------------------------------------------

def test_the_wide_form():
    assert wg.WIDE_FORM == (48, 16, (32, 48), False) and "wide" not in gc.FORMS and len(gc.CASES) == 37
    assert set(wg.FAMILIES) == {"rotated", "lateral", "arc", "behind", "rotation", "still", "far", "anchor", "fx1400"}
    assert len({c.seed for c in wg.GEOMETRY.values()}) == len(wg.GEOMETRY) == len(wg.FAMILIES)
    assert not {c.seed for c in wg.GEOMETRY.values()} & {c.seed for c in gc.CASES.values()}


@pytest.mark.parametrize("name", list(wg.GEOMETRY))
def test_every_wide_geometry_case_meets_its_conditions(name):
    """tests/test_geometry_cases.py's conditions.  Seen: spread at most 9.8e-13 in the five measures (far_wide) and 5.7e-14 on gamma
    (anchor_wide); rank margins from 24 up (still_wide; 2e9 and more on the rank-3 families); gate margins from 1.5e-2 up; 8 - 15
    of 16 tracks accepted; 326 views behind the camera (behind_wide)."""
    case = wg.GEOMETRY[name]
    prob, ref = wg.geometry(name)
    N, F, views, _ = wg.WIDE_FORM
    M = wc.views(prob)
    assert (prob.N, prob.F) == (N, F) and M.min() >= views[0] and M.max() <= views[1] and wc.wide(prob).all()
    tab = table(name)
    ranks, worst = Counter(), np.inf
    for j, (qr, (rk, sm), _) in enumerate(tab):
        assert qr.rank == rk, (name, j, qr.rank, rk)
        assert qr.margin >= gc.RANK_FACTOR and sm >= gc.RANK_FACTOR, (name, j, qr.margin, sm)
        worst = min(worst, qr.margin, sm)
        ranks[rk] += 1
    want = 2 if case.exact_rank2 else 3
    assert set(ranks) == {want}, (name, ranks)
    from scipy.stats import chi2
    assert ref["status"] == 0 and np.array_equal(ref["crit"], chi2.ppf(0.95, 2 * M - want))
    n_acc = int(ref["accepted"].sum())
    margin = wc.margin(ref)
    spread, gspread = gc.second_form(prob, ref)
    orders = Counter(t[0].order for t in tab if t[0].counted)
    print(f"WIDEGEOMETRY {name}: seed {case.seed} pivot orders {dict(orders)} ranks {dict(ranks)} rank margin {worst:.1e} | accepted {n_acc} / {F}, "
          f"gate margin {margin:.1e} | spread " + " ".join(f"{x:.1e}" for x in spread) + f" gamma {gspread:.1e} | views behind {prob.meta['views_behind']}")
    assert margin >= gc.GATE_MARGIN, (name, margin)
    assert 1 <= n_acc <= F - 1, (name, n_acc)
    assert max(spread) <= gc.SPREAD and gspread <= gc.SPREAD, (name, spread, gspread)
    if case.family == "behind":
        assert prob.meta["views_behind"] > 0
    else:
        assert prob.meta["views_behind"] == 0
    if case.exact_rank2:                                       # the tracks on which K2's pivoting decides the rank
        hz = np.nonzero(prob.meta["horizon"])[0]
        assert len(hz) >= 1 and np.abs(prob.idp_m[hz, 2]).max() <= 2e-3, (name, len(hz))
    if case.family == "rotated":
        assert not np.array_equal(prob.cam_R0, prob.cam_R) and abs(prob.gravity[2] + 9.81) > 1e-3
    if case.family == "fx1400":
        assert prob.K[0, 0] == 1400.0
    if case.family == "anchor":
        assert min(np.min(np.linalg.norm(prob.cam_t - b, axis=1)) for b in prob.idp_base) > 0.01        # the base is off every clone
    if case.family == "still":
        assert np.all(prob.cam_t == prob.cam_t[0]) and np.all(prob.cam_R == prob.cam_R[0])


def test_wide_geometry_reaches_every_pivot_order_and_a_view_behind():
    """Seen: rank 3 {(2, 1, 0): 47, (1, 2, 0): 34, (0, 1, 2): 14, (2, 0, 1): 13, (0, 2, 1): 3, (1, 0, 2): 1}; rank 2, the two columns
    taken {(2, 1): 11, (2, 0): 8, (0, 2): 7, (1, 2): 6}; the wide tracks of tests/wide_cases.py {(1, 2, 0): 9, (2, 1, 0): 5, (0, 2, 1): 4}
    (the last on its rank-2 batch: columns 0 and 2 taken)."""
    total = Counter()
    for name, c in wg.GEOMETRY.items():
        if not c.exact_rank2:
            total += Counter(t[0].order for t in table(name) if t[0].counted and t[0].rank == 3)
    two = Counter()
    for name, c in wg.GEOMETRY.items():
        if c.exact_rank2:
            two += Counter(t[0].order[:2] for t in table(name) if t[0].counted)
    print(f"WIDEGEOMETRY pivots: rank 3 {dict(total)} | rank 2, first two columns {dict(two)}")
    for o in gc.ORDERS:
        assert total[o] >= 1, (o, total)
    assert len(two) >= 3, two
    assert sum(wg.geometry(n)[0].meta["views_behind"] > 0 for n in wg.GEOMETRY) >= 1
    # what the batches of tests/wide_cases.py reach: three orders
    old = Counter()
    for prob in (wc.synth_case("first")[0], wc.synth_case("cap")[0], wc.synth_case("mixed")[0], wc.reversed_case()[0], wc.rank2_case()[0]):
        old += Counter(t[0].order for j, t in enumerate(gc.track_table(prob)) if wc.wide(prob)[j])
    print(f"WIDEGEOMETRY pivots of tests/wide_cases.py: {dict(old)}")
    assert len(set(old)) == 3 and set(old) < set(total)
