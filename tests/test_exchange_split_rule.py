"""CPU tests of the whole-batch rule for split records (`msckf_exchange_split_rule`, no engine, no GPU): its answers are
those of a NumPy mirror of the classification, and they do not depend on which rank asks."""
import numpy as np
import pytest

from msckf_amd import synth
from msckf_amd.api import exchange_split_rule
from msckf_amd.shard import partition_features, shard_group_flags


def _mirror(prob, shards):
    """NumPy count: per long track (span > 10 slots) its view groups as msckf_set_features cuts them -- ceil(span / 10)
    stretches of equal width, empty ones skipped --, 3 rows per group (3 (groups - 1) when H_f has full rank); the
    first slots of short tracks and of the narrow blocks (groups of 2+ views)."""
    vp = np.asarray(prob.view_ptr)
    sl = np.asarray(prob.obs_slot).reshape(-1)
    N = prob.N
    rows = np.zeros(len(shards), dtype=np.int64)
    flags = np.zeros((len(shards), N), dtype=np.uint8)
    span_after = 0
    for r, (lo_f, hi_f) in enumerate(shards):
        for f in range(lo_f, hi_f):
            s = sl[vp[f]:vp[f + 1]]
            lo, hi = int(s.min()), int(s.max())
            span = hi - lo + 1
            if span <= 10:
                flags[r, lo] = 1
                span_after = max(span_after, span)
                continue
            ng0 = -(-span // 10)
            cuts = [lo + ((g + 1) * span) // ng0 for g in range(ng0)]
            grp = np.searchsorted(cuts, s, side="right")
            ng = 0
            for g in range(ng0):
                v = s[grp == g]
                if len(v) == 0:
                    continue
                ng += 1
                if len(v) >= 2:
                    flags[r, v[0]] = 1
                    span_after = max(span_after, int(v[-1] - v[0] + 1))
            rows[r] += 3 * ng
    return rows, flags, span_after


@pytest.mark.parametrize("N,F,M,S,seed", [(30, 300, 30, 2, 1), (30, 300, 30, 8, 2), (30, 600, 30, 4, 3), (50, 300, 31, 4, 4),
                                          (31, 64, 31, 3, 5), (20, 120, 20, 5, 6)])
def test_rule_matches_the_numpy_count(N, F, M, S, seed):
    prob = synth.make_problem(N, F, M, seed=seed, variable_tracks=True, min_track=2)
    shards = partition_features(prob.view_ptr, S)
    rule = exchange_split_rule(prob, shards)
    rows, flags, span_after = _mirror(prob, shards)
    assert rule["split"]
    assert rule["rows"] == -(-int(rows.max()) // 16) * 16 and rule["total"] == int(rows.sum())
    assert rule["span"] == span_after <= 10
    assert np.array_equal(rule["flags"], flags)


def test_every_rank_gets_the_same_answer():
    """Every rank passes the whole batch and the partition: the answer is a function of them only (here: asked in
    rank order and in reverse, repeatedly)."""
    prob = synth.few_long_tracks_problem(30, 2000, 10, 10, seed=7)
    shards = partition_features(prob.view_ptr, 8)
    answers = [exchange_split_rule(prob, shards) for _ in list(range(8)) + list(reversed(range(8)))]
    for a in answers[1:]:
        assert a["split"] == answers[0]["split"] and a["span"] == answers[0]["span"]
        assert a["rows"] == answers[0]["rows"] and a["total"] == answers[0]["total"]
        assert np.array_equal(a["flags"], answers[0]["flags"])
    assert answers[0]["split"] and answers[0]["total"] == 90 and answers[0]["rows"] == 96


def test_batches_the_rule_does_not_split():
    # no long track
    p = synth.make_problem(30, 200, 10, seed=8)
    r = exchange_split_rule(p, partition_features(p.view_ptr, 2))
    assert not r["split"] and r["span"] == 10 and r["rows"] == 0
    assert np.array_equal(r["flags"], shard_group_flags(p, partition_features(p.view_ptr, 2)))
    # more than 31 views
    p = synth.make_problem(40, 60, 35, seed=9, variable_tracks=True, min_track=20)
    assert not exchange_split_rule(p, partition_features(p.view_ptr, 2))["split"]
    # views out of slot order
    p = synth.make_problem(24, 40, 24, seed=10, variable_tracks=True, min_track=12)
    sl = p.obs_slot.copy()
    a, b = int(p.view_ptr[0]), int(p.view_ptr[1])
    sl[a:b] = sl[a:b][::-1].copy()
    p.obs_slot = sl
    assert not exchange_split_rule(p, partition_features(p.view_ptr, 2))["split"]
    # mostly 11 - 15-slot tracks and none longer (BASELINE configs[4]): the 90-column pipeline
    p = synth.make_problem(50, 300, 15, seed=11)
    r = exchange_split_rule(p, partition_features(p.view_ptr, 4))
    assert not r["split"] and r["span"] == 15
    # more remainder rows than K6-K7 takes as they are (3840 at N = 30)
    p = synth.make_problem(30, 1200, 30, seed=12, variable_tracks=True, min_track=20)
    assert not exchange_split_rule(p, partition_features(p.view_ptr, 4))["split"]


def test_bad_arguments_are_refused():
    from msckf_amd import _ffi
    p = synth.make_problem(30, 50, 30, seed=13, variable_tracks=True, min_track=2)
    with pytest.raises(_ffi.EngineError):
        exchange_split_rule(p, [(0, 20), (20, 40)])          # the shards do not cover the batch


def test_the_rule_and_the_shards_intake_agree():
    """A sharded update is right only if the whole-batch rule on every rank and msckf_set_features on every shard cut the same
    tracks the same way.  Both take their rules from csrc/batch_order.h; here the library's rule is held against what
    batch_order_model.py derives from the BatchOrder of every shard (the model test_batch_order.py holds the header to), on the
    random batches of that test that have no unsplittable long track, cut into two to four shards."""
    import random
    from types import SimpleNamespace
    from batch_order_model import (RANDOM_N, REM_DIRECT_MID, SPLIT_SPAN, WIDE_SPAN, Order, batch, batch_lines, random_batches,
                                   splittable, tracks)
    n_split = n_whole = 0
    for N in RANDOM_N:
        rng = random.Random(2000 + N)
        for b in random_batches(N, random.Random(1000 + N)):
            trk = tracks(b)
            F = len(trk)
            span = [max(t) - min(t) + 1 for t in trk]
            if F < 4 or any(s > WIDE_SPAN and not splittable(t) for s, t in zip(span, trk)):
                continue
            S = rng.randint(2, 4)
            cuts = [0] + sorted(rng.sample(range(1, F), S - 1)) + [F]
            shards = list(zip(cuts, cuts[1:]))
            vp = np.asarray(b["view_ptr"], dtype=np.int32)
            prob = SimpleNamespace(N=N, F=F, view_ptr=vp, obs_slot=np.asarray(b["obs_slot"], dtype=np.int32))
            rule = exchange_split_rule(prob, shards)

            def shard_orders(split):
                out = []
                for lo_f, hi_f in shards:
                    o = Order()
                    sub = batch(N, vp[lo_f:hi_f + 1] - vp[lo_f], b["obs_slot"][vp[lo_f]:vp[hi_f]], maxM=40, split=split, rem=1 << 20)
                    assert batch_lines(sub, o)[3] == "build 0"
                    out.append((o, hi_f - lo_f))
                return out
            # the whole batch's decision (library defaults): the window must fit K6-K7's dense block update (N = 65 does not), most
            # tracks must not be 11 - 15-slot ones with none longer, K6-K7 must take all remainder rows as they are
            n_mid, n_long = sum(WIDE_SPAN < s <= SPLIT_SPAN for s in span), sum(s > SPLIT_SPAN for s in span)
            direct = 16384 if 6 * N > 186 else 3840
            keep = n_long == 0 and (2 * n_mid > F or 6 * n_mid > (direct if 6 * N > 186 else min(direct, REM_DIRECT_MID)))
            total = sum(o.rem_cap for o, _ in shard_orders(1))
            want = 10 < N <= 37 and n_mid + n_long > 0 and not keep and total <= direct
            assert rule["split"] == want, (N, text_of(b))
            orders = shard_orders(int(want))
            band = [o.entries[:n - o.Fw] + o.entries[n:n + o.nNarrow] for o, n in orders]      # short tracks and narrow blocks
            assert rule["span"] == max(e["hi"] - e["lo"] + 1 for es in band for e in es)
            assert rule["rows"] == -(-max(o.rem_cap for o, _ in orders) // 16) * 16 and rule["total"] == sum(o.rem_cap for o, _ in orders)
            flags = np.zeros((S, N), dtype=np.uint8)
            for r, es in enumerate(band):
                flags[r, [e["lo"] for e in es]] = 1
            assert np.array_equal(rule["flags"], flags)
            n_split += want
            n_whole += not want
    assert n_split > 20 and n_whole > 20


def text_of(b):
    return " ".join(map(str, b["view_ptr"])) + " | " + " ".join(map(str, b["obs_slot"]))
