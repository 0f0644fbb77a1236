"""What the sweep kernels rely on in the host's schedules and tables (`csrc/sweep_plan.h`), stated on its own, and the table
that satisfies each statement minimally.  `test_sweep_plan.py` compares `sweep_plan_driver.cpp`'s output with it.

A node is (wtot, nf, adopt, gate, rc, folds), a fold (off, w, ew, prod, ld).  An adopted first fold is copied into the empty R
and runs no step; the others are the node's scheduled folds, fold j of them on fold slot j % nf.

schedule   an adopted fold has t0 = 0.  The first scheduled fold starts at step 1.  Fold g starts at least
           off[g] - off[g-1] + 1 steps after fold g-1 (a step of a fold touches one row of R, the row of its pivot column) and
           no sooner than t0[g-nf] + ew[g-nf] + 1 (its wavefront is free); t0 is the smallest such step; nsteps the largest
           t0 + ew.
flush      a fold runs one step per envelope column: at step t in [t0, t0 + ew) its pivot row is off + t - t0.  The rows
           final at the head of step t are those below the smallest pivot row any unfinished fold has now or will have first;
           entry t = lo | n << 16 with lo the sum of the earlier n; entry nsteps completes wtot.  The ring verdict is false
           exactly when a row touched in a step lies rc or more beyond what was flushed before the step, or the adopted
           triangle does not fit rc rows.
gate       k_sweep.h's fetch rule gives a multiset of requirements (step, producer, rows); the table holds each exactly once, at
           a step no later than its own and at its own unless that entry is full, at most two per entry of 12 bits each,
           entry 0 empty, the step-0 list behind the nsteps + 2 entries.
publish    what was final WS_PUB_LAG + 1 steps earlier, where that count passes a boundary of the 16-row blocks that end at
           wtot; never decreasing.
memo       the first CAP distinct keys take the slots in order, then the oldest is replaced; a hit is the entry itself."""
import numpy as np

WS_PUB_LAG = 4
MEMO_CAP = 64


def scheduled(node):
    """Index of the first scheduled fold."""
    return 1 if node["adopt"] and node["folds"] else 0


def schedule(node):
    folds, nf, first = node["folds"], node["nf"], scheduled(node)
    t0 = [0] * len(folds)
    for g in range(first, len(folds)):
        need = [1]
        if g > first:
            need = [t0[g - 1] + folds[g][0] - folds[g - 1][0] + 1]
        if g - first >= nf:
            need.append(t0[g - nf] + folds[g - nf][2] + 1)
        t0[g] = max(need)
    return t0, max([t0[g] + folds[g][2] for g in range(first, len(folds))], default=0)


def flush(node, t0, nsteps):
    """(entries, cumulative counts, ring verdict)"""
    folds, wtot, rc, first = node["folds"], node["wtot"], node["rc"], scheduled(node)
    t = np.arange(nsteps + 1)[:, None]
    off = np.array([f[0] for f in folds[first:]], dtype=np.int64)[None, :]
    ew = np.array([f[2] for f in folds[first:]], dtype=np.int64)[None, :]
    s = np.array(t0[first:], dtype=np.int64)[None, :]
    unfinished = t < s + ew
    running = unfinished & (t >= s)
    pivot = off + np.maximum(t - s, 0)
    count = np.where(unfinished, pivot, wtot).min(axis=1, initial=wtot)
    assert count[nsteps] == wtot and (np.diff(count) >= 0).all() and (count >= 0).all()
    lo = np.concatenate([[0], count[:-1]])
    entries = (lo | ((count - lo) << 16)).tolist()
    far = np.where(running, pivot, -1).max(axis=1, initial=-1)
    ok = not (far >= lo + rc).any()
    if first == 1 and folds[0][0] + folds[0][1] > rc:
        ok = False
    return entries, count.tolist(), ok


def requirements(node, t0, nsteps):
    """[(step, word)] of the fetch rule: rows [0, 8) of a fold's source before step 0 (the first nf scheduled folds) or in chunk
    max((ew' - 1) / 8 - 1, 0) of the fold that holds the slot before it; rows [8 KK + 8, 8 KK + 16) at the head of chunk KK."""
    folds, nf, first = node["folds"], node["nf"], scheduled(node)
    out = []
    for g in range(first, len(folds)):
        off, w, ew, prod, ld = folds[g]
        if prod <= 0:
            continue
        step = 0
        if g - first >= nf:
            q = folds[g - nf]
            step = t0[g - nf] + 8 * max((q[2] - 1) // 8 - 1, 0)
        out.append((min(step, nsteps), (prod - 1) << 6 | min(w, 8)))
        for kk in range(8):
            if 8 * kk < ew and 8 * kk + 8 < w:
                out.append((min(t0[g] + 8 * kk, nsteps), (prod - 1) << 6 | min(w, 8 * kk + 16)))
    return out


def check_gate(node, t0, nsteps, n0, words):
    """The driver's gate table against the requirements.  Returns how many sit at an earlier step than their own."""
    assert len(words) == nsteps + 2 + n0
    assert words[0] == 0
    placed = [(0, r) for r in words[nsteps + 2:]]
    full = set()
    for t in range(1, nsteps + 2):
        a, b = words[t] & 0xFFF, words[t] >> 12
        assert 0 <= b <= 0xFFF and (a != 0 or b == 0), (t, words[t])
        placed += [(t, r) for r in (a, b) if r]
        if b:
            full.add(t)
    want = requirements(node, t0, nsteps)
    assert all(0 < r <= 0xFFF for _, r in want)
    assert sorted(r for _, r in placed) == sorted(r for _, r in want)
    moved = 0
    for r in set(r for _, r in want):                      # equal words: the k-th placed serves the k-th wanted
        for at, own in zip(sorted(t for t, x in placed if x == r), sorted(t for t, x in want if x == r)):
            assert at <= own, (r, at, own)
            if at < own:                                  # moved only off a full entry, and over full entries only
                moved += 1
                assert all(t in full for t in range(max(at, 0) + 1, own + 1)), (r, at, own)
    return moved


def publish(node, counts, nsteps):
    boff = (16 - node["wtot"] % 16) % 16
    out, published = [], 0
    for t in range(nsteps + 1):
        rows = counts[t - WS_PUB_LAG - 1] if t > WS_PUB_LAG else 0
        if (rows + boff) // 16 > (published + boff) // 16:
            out.append(rows)
            published = rows
        else:
            out.append(0)
    assert [x for x in out if x] == sorted(set(x for x in out if x))
    return out


class Memo:
    def __init__(self):
        self.keys, self.next = [], 0

    def clear(self):
        self.keys = []                                     # (the cursor stays)

    def look(self, node):
        """(slot, hit)"""
        key = (node["wtot"], node["nf"], bool(node["adopt"]), bool(node["gate"]), tuple(map(tuple, node["folds"])))
        if key in self.keys:
            return self.keys.index(key), 1
        if len(self.keys) < MEMO_CAP:
            self.keys.append(key)
            return len(self.keys) - 1, 0
        slot, self.next = self.next, (self.next + 1) % MEMO_CAP
        self.keys[slot] = key
        return slot, 0


def words(name, xs):
    return " ".join([name] + [str(int(x)) for x in xs])


def node_lines(node, block, memo):
    """The lines the driver prints for `node`, its gate line taken from `block` once check_gate has passed it.  Returns
    (lines, how many requirements moved to an earlier step, ring verdict)."""
    t0, nsteps = schedule(node)
    entries, counts, ok = flush(node, t0, nsteps)
    gate = [int(x) for x in block[3].split()[1:]]
    moved = check_gate(node, t0, nsteps, gate[0], gate[1:])
    slot, hit = memo.look(node)
    tab = entries + (gate[1:] if node["gate"] else [])
    lines = [words("t0", t0), "nsteps %d" % nsteps, words("flush %d" % ok, entries), block[3],
             words("publish", publish(node, counts, nsteps)), "memo %d %d" % (slot, hit),
             words("tables %d %d" % (nsteps, gate[0] if node["gate"] else -1), t0) + words(" :", tab), "end"]
    return lines, moved, ok
