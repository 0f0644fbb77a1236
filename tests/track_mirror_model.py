"""The host mirror of the track store (`csrc/track_mirror.h`) restated with dicts and lists, in the manner of
`track_events.replay`: what DESIGN.md 3.8 says the mirror does, and the text `tests/track_mirror_driver.cpp` prints for it.
Not a conftest: imported by name.

`live` maps id -> dict(row, slots, anchor, lost, tracked, desc), in creation order (a dict keeps insertion order: the
reference's `feature_tracks`).  `free` is the stack of free rows, the last element goes out next."""

OK, ERR_ARG, ERR_DUP_SLOT = 0, -1, -6
FAILED = (1, 2)                             # result bytes of a failed epipolar / homography test


class Model:
    def __init__(self):
        self.T = self.V = 0
        self.clear()

    # ---- operations: each returns (rc, bad pair or -1, rows listed or None) -------------------------------------------
    def size(self, T, V):
        self.T, self.V = T, V
        self.clear()
        return OK, -1, None

    def clear(self):
        self.live, self.dropped = {}, []
        self.free = list(range(self.T))[::-1]                       # row 0 goes out first
        return OK, -1, None

    def check(self, ids, finite, newest):
        """(rc, bad, offenders, reason): every pair that offends on its own, and what the first of them decides."""
        off = []
        for i, fid in enumerate(ids):
            t = self.live.get(fid)
            if fid < 0 or not finite[i]:
                off.append((i, ERR_ARG, "arg"))
            elif fid in ids[:i]:
                off.append((i, ERR_DUP_SLOT, "repeat"))
            elif t is not None and t["slots"] and t["slots"][-1] == newest:
                off.append((i, ERR_DUP_SLOT, "newest"))
            elif t is not None and len(t["slots"]) == self.V:
                off.append((i, ERR_ARG, "row"))
        if off:
            return off[0][1], off[0][0], [o[0] for o in off], off[0][2]
        fresh = [i for i, fid in enumerate(ids) if fid not in self.live]
        if len(fresh) > len(self.free):                              # counted after the pairs
            return ERR_ARG, fresh[len(self.free)], [], "store"
        return OK, -1, [], None

    def intake(self, ids, finite, res, newest, frame, with_desc):
        """`observe` (frame False: every pair is an append without a descriptor) or a frame with its result bytes."""
        rc, bad, self.offenders, self.reason = self.check(ids, finite, newest)
        self.created = self.appended = self.fresh_failed = 0
        if rc != OK:
            return rc, bad, None
        for fid, r in zip(ids, res):
            if fid not in self.live:
                self.live[fid] = dict(row=self.free.pop(), slots=[], anchor=newest, lost=0, tracked=0, desc=int(frame and with_desc))
                self.created += 1
                self.fresh_failed += int(frame and r in FAILED)
            t = self.live[fid]
            if frame and r in FAILED:
                t["lost"] += 1
                continue
            if not (frame and with_desc):
                t["desc"] = 0
            t["slots"].append(newest)
            t["tracked"] += 1
            t["lost"] = 0
            self.appended += 1
        if frame:
            for fid, t in self.live.items():
                if fid not in ids:
                    t["lost"] += 1
        return OK, -1, None

    def remove(self, ids):
        if len(set(ids)) != len(ids) or any(fid not in self.live for fid in ids):
            return ERR_ARG, -1, None
        for fid in ids:
            self.free.append(self.live.pop(fid)["row"])
        return OK, -1, None

    def drop(self, mask):
        new = {}
        for s, gone in enumerate(mask):
            new[s] = -1 if gone else len([x for x in new.values() if x >= 0])
        self.dropped = []
        for fid, t in sorted(self.live.items(), key=lambda e: e[1]["row"]):
            t["slots"] = [new[s] for s in t["slots"] if new[s] >= 0]
            if t["anchor"] >= 0:
                t["anchor"] = new[t["anchor"]]
            if not t["slots"]:
                self.dropped.append(fid)
                self.free.append(self.live.pop(fid)["row"])
        return OK, -1, None

    def rows(self):
        return OK, -1, sorted(t["row"] for t in self.live.values())

    def created_order(self, want=None):
        return OK, -1, [t["row"] for t in self.live.values() if want is None or any(want[s] for s in t["slots"])]

    def ids_created_order(self):
        return list(self.live)

    # ---- the driver's text ------------------------------------------------------------------------------------------------
    def dump(self):
        def row(words, xs):
            return " ".join([words] + [str(x) for x in xs])
        out = ["%s | %s | %s" % ("tracks %d views %d" % (len(self.live), sum(len(t["slots"]) for t in self.live.values())),
                                 row("free", self.free), row("dropped", self.dropped))]
        rank = {fid: k for k, fid in enumerate(self.live)}
        for fid in sorted(self.live):
            t = self.live[fid]
            out.append(row("id %d row %d anchor %d lost %d tracked %d rank %d desc %d slots"
                           % (fid, t["row"], t["anchor"], t["lost"], t["tracked"], rank[fid], t["desc"]), t["slots"]))
        return out + ["end"]

    def run(self, line):
        """One script line -> the lines the driver prints for it."""
        w = line.split()
        op, a = w[0], [int(x) for x in w[1:]]
        if op == "size":
            rc, bad, rows = self.size(*a)
        elif op == "clear":
            rc, bad, rows = self.clear()
        elif op == "observe":
            n = a[1]
            rc, bad, rows = self.intake(a[2:2 + n], [1] * n, [0] * n, a[0], False, False)
        elif op == "frame":
            t = a[3:3 + 3 * a[2]]
            rc, bad, rows = self.intake(t[0::3], t[1::3], t[2::3], a[0], True, bool(a[1]))
        elif op == "remove":
            rc, bad, rows = self.remove(a[1:1 + a[0]])
        elif op == "drop":
            rc, bad, rows = self.drop(a[1:1 + a[0]])
        elif op == "rows":
            rc, bad, rows = self.rows()
        elif op == "created":
            rc, bad, rows = self.created_order()
        elif op == "where":
            rc, bad, rows = self.created_order(a[1:1 + a[0]])
        else:
            raise ValueError(line)
        out = ["rc %d bad %d" % (rc, bad)]
        if rows is not None:
            out.append(" ".join(["rows"] + [str(r) for r in rows]))
        return out + self.dump()
