"""What `csrc/batch_order.h` is meant to compute, with lists and sorts: the text `batch_order_driver.cpp` prints for a script of
batches.  The view groups are `failing_batches.view_groups`; nothing here reads the driver's output.

A batch is a dict: N, maxM, split (the context's verdict), direct_cap and wide (the remainder rows K6-K7 takes as they are, the
window wider than k_fold keeps in LDS), rem (the remainder rows a split record takes, -1: no split records), rec_cap (-1: the
raw layout's), nch (ranges of the scan), view_ptr, obs_slot."""
import numpy as np

from failing_batches import SPLIT_SLOTS, SPLIT_SPAN, WIDE_SPAN, REM_DIRECT_MID, view_groups

SPLIT_MAXG, SPLIT_MAXM = 6, 31
OK, ERR_ARG, ERR_DUP_SLOT = 0, -1, -6
BUILT, RECORD_CAPACITY, REMAINDER_CAPACITY = 0, 1, 2
GATHER_REC, SPLIT_REC, FEAT_INFO = 24, 40, 32


def batch(N, view_ptr, obs_slot, maxM=None, split=None, direct_cap=3840, wide=None, rem=-1, rec_cap=-1, nch=1):
    M = np.diff(view_ptr)
    return dict(N=N, maxM=int(max(M.max(), 1)) if maxM is None else maxM, split=int(N > WIDE_SPAN if split is None else split),
                direct_cap=direct_cap, wide=int(6 * N > 186 if wide is None else wide), rem=rem, rec_cap=rec_cap, nch=nch,
                view_ptr=[int(x) for x in view_ptr], obs_slot=[int(x) for x in obs_slot])


def text(b):
    head = "batch %d %d %d %d %d %d %d %d %d" % (b["N"], b["maxM"], b["split"], b["direct_cap"], b["wide"], b["rem"], b["rec_cap"],
                                                 b["nch"], len(b["view_ptr"]) - 1)
    return " ".join([head] + [str(x) for x in b["view_ptr"]] + [str(x) for x in b["obs_slot"]])


def tracks(b):
    vp = b["view_ptr"]
    return [b["obs_slot"][vp[f]:vp[f + 1]] for f in range(len(vp) - 1)]


def track_error(b, f):
    """The code of track f alone: the first offending view decides."""
    vp, N = b["view_ptr"], b["N"]
    M = vp[f + 1] - vp[f]
    if M < 1 or M > b["maxM"]:
        return ERR_ARG
    seen = set()
    for sl in b["obs_slot"][vp[f]:vp[f + 1]]:
        if sl < 0 or sl >= N:
            return ERR_ARG
        if sl in seen:
            return ERR_DUP_SLOT
        seen.add(sl)
    return OK


def scan(b):
    """The first failing track of the lowest failing range -- which is the first failing track."""
    for f in range(len(b["view_ptr"]) - 1):
        rc = track_error(b, f)
        if rc != OK:
            return rc
    return OK


def splittable(sl):
    span = max(sl) - min(sl) + 1
    return (span > WIDE_SPAN and all(a < c for a, c in zip(sl, sl[1:])) and len(sl) <= SPLIT_MAXM
            and -(-span // SPLIT_SLOTS) <= SPLIT_MAXG)


def align(x, a):
    return -(-x // a) * a


class Order:
    """What a context keeps of its last batch."""
    lines = ["order invalid"]


def batch_lines(b, order, seen=None):
    """The driver's block for batch b; `order` carries the BatchOrder from batch to batch.  seen: a dict of branch counters."""
    seen = seen if seen is not None else {}

    def met(name, n=1):
        seen[name] = seen.get(name, 0) + n
    N, F = b["N"], len(b["view_ptr"]) - 1
    rc = scan(b)
    out = ["rc %d" % rc]
    if rc != OK:
        return out + order.lines + ["end"]          # the scan touches no BatchOrder
    trk = tracks(b)
    M = [len(t) for t in trk]
    lo, hi = [min(t) for t in trk], [max(t) for t in trk]
    span = [h - l + 1 for l, h in zip(lo, hi)]
    cls = [2 if b["split"] and splittable(t) else 0 for t in trk]
    n_long = sum(s > SPLIT_SPAN for s in span)
    n_mid = sum(WIDE_SPAN < s <= SPLIT_SPAN for s in span)
    met("unsplittable long", sum(1 for s, k in zip(span, cls) if b["split"] and s > WIDE_SPAN and k == 0))
    met("N > 64", int(N > 64))
    mid_cap = b["direct_cap"] if b["wide"] else min(b["direct_cap"], REM_DIRECT_MID)
    most, many = 2 * n_mid > F, 6 * n_mid > mid_cap
    keep = 2 in cls and b["rem"] < 0 and n_long == 0 and (most or many)
    if keep:
        met("override: most tracks", int(most))
        met("override: too many rows", int(many))
        met("override: only most tracks", int(most and not many))
        met("override: only too many rows", int(many and not most))
        cls = [0] * F
    mmax = [max([m for m, k in zip(M, cls) if k == c], default=0) for c in (0, 1, 2)]
    out.append("scan Mmax %d %d %d mid %d long %d keep %d" % (mmax[0], mmax[1], mmax[2], n_mid, n_long, keep))
    out.append("key " + " ".join(str(k * N * N + l * N + h) for k, l, h in zip(cls, lo, hi)))
    met("class 2", cls.count(2))
    # the stable sort by (class, first slot, last slot)
    perm = sorted(range(F), key=lambda f: (cls[f], lo[f], hi[f]))
    Fb = cls.count(0)
    narrow, wide, split = [], [], []
    for sidx in range(Fb, F):
        f = perm[sidx]
        groups = view_groups(np.asarray(trk[f]))
        met("empty stretch", int(len(groups) < -(-span[f] // SPLIT_SLOTS)))
        met("one-view group", sum(1 for v0, v1 in groups if v1 - v0 == 1))
        for g, (v0, v1) in enumerate(groups):
            if v1 - v0 >= 2:
                narrow.append(dict(parent=sidx, f=f, a=b["view_ptr"][f] + v0, M=v1 - v0, lo=trk[f][v0], hi=trk[f][v1 - 1], pi=sidx - Fb, g=g))
        wide.append(dict(parent=sidx, f=f, a=b["view_ptr"][f], M=M[f], lo=lo[f], hi=hi[f], pi=sidx - Fb, g=-1))
        split.append(dict(child=[-1] * SPLIT_MAXG, gv=[v0 for v0, _ in groups] + [M[f]] + [0] * (SPLIT_MAXG - len(groups)), ng=len(groups)))
    narrow.sort(key=lambda k: (k["lo"], k["hi"]))
    rem_cap = sum(3 * s["ng"] for s in split)
    sum_m = b["view_ptr"][F]
    rec_cap = 2 * F + sum_m // 2 + 8
    fail = BUILT
    if F + len(narrow) + len(wide) > (rec_cap if b["rec_cap"] < 0 else b["rec_cap"]):
        fail = RECORD_CAPACITY
        met("record capacity")
    elif split and b["rem"] >= 0 and rem_cap > b["rem"]:
        fail = REMAINDER_CAPACITY
        met("remainder capacity")
    out.append("build %d" % fail)
    if fail != BUILT:
        order.lines = ["order invalid"]              # build() reports the value invalid
        return out + order.lines + ["end"]
    # the entries: the F tracks, the narrow blocks, the remainder blocks; a split track has no K4 block of its own
    entries = [dict(f=f, a=b["view_ptr"][f], M=M[f], lo=lo[f], hi=hi[f], rows=0 if s >= Fb and split else 2 * M[f]) for s, f in enumerate(perm)]
    for k in narrow:
        split[k["pi"]]["child"][k["g"]] = len(entries)
        entries.append(dict(k, rows=2 * k["M"]))
    for k in wide:
        split[k["pi"]]["wide"] = len(entries)
        entries.append(dict(k, rows=3 * SPLIT_MAXG))
    Fs = len(entries)
    view, blk = [0], [0]
    for e in entries:
        view.append(view[-1] + e["M"])
        blk.append(blk[-1] + (6 * e["M"] + 1) * e["rows"])
    sum_ms = view[-1]
    o = ["order Fb %d Fw %d Fs %d nNarrow %d sumMs %d split_on %d rem_cap %d Mmax %d %d %d stack %d"
         % (Fb, F - Fb, Fs, len(narrow), sum_ms, bool(split), rem_cap, max(mmax), mmax[0], mmax[2], blk[-1])]
    o.append(" ".join(["perm"] + [str(f) for f in perm]))
    o.append(" ".join(["view"] + [str(v) for v in view]))
    o.append(" ".join(["fmin"] + [str(e["lo"]) for e in entries]))
    o.append(" ".join(["fmax"] + [str(e["hi"]) for e in entries]))
    o.append(" ".join(["parent"] + [str(e["parent"]) for e in entries[F:]]))
    for s in split:
        o.append("split %s wide %d gv %s ng %d rows %d" % (" ".join(map(str, s["child"])), s["wide"], " ".join(map(str, s["gv"])), s["ng"], 3 * s["ng"]))
    order.lines = o
    order.Fs, order.nNarrow, order.Fw, order.rem_cap, order.entries, order.perm = Fs, len(narrow), F - Fb, rem_cap, entries, perm
    out += o
    out.append(" ".join(["rec"] + ["%d %d %d %d %d" % (e["f"], e["a"], e["M"], v, 0 if e["rows"] == 0 else k)
                                   for e, v, k in zip(entries, view, blk)]))
    # the raw image: [uv | base | m | rho | slot] padded to 16, the records, the split records
    raw = [0, 16 * sum_m, 16 * sum_m + 24 * F, 16 * sum_m + 48 * F, 16 * sum_m + 56 * F]
    raw_bytes = align(raw[4] + 4 * sum_m, 16)
    out.append("raw %d %d %d %d %d bytes %d rec_cap %d pin %d split_off %d"
               % (*raw, raw_bytes, rec_cap, raw_bytes + rec_cap * GATHER_REC + (F + 1) * SPLIT_REC, raw_bytes + align(Fs * GATHER_REC, 16)))
    # the sorted image: [uv | base | m | rho | blk | view | perm | slot | fmin | info]
    so = [0, 16 * sum_ms]
    for size in (24 * Fs, 24 * Fs, 8 * Fs, 8 * Fs, align(4 * (Fs + 1), 8), align(4 * Fs, 8), align(4 * sum_ms, 8)):
        so.append(so[-1] + size)
    so.append(align(so[-1] + 4 * Fs, 16))
    out.append("sorted %s bytes %d" % (" ".join(map(str, so)), so[-1] + FEAT_INFO * Fs))
    order.raw, order.raw_bytes, order.rec_cap, order.sorted = raw, raw_bytes, rec_cap, so
    return out + ["end"]


# ---- the batches of the tests (test_batch_order.py, test_exchange_split_rule.py) ----------------------------------------------
RANDOM_N, N_RANDOM = (11, 12, 16, 31, 37, 65), 60


def random_track(rng, N, maxM, kind):
    """Slots of one track.  short: within 10 slots; mid: 11 - 15; long: more; sparse: long with few views (stretches without a
    view, one-view groups); full: every slot of its span (more than 31 views where maxM allows); unordered: long, views shuffled."""
    if kind == "short" or N <= WIDE_SPAN:
        span = rng.randint(1, min(WIDE_SPAN, N))
    elif kind == "mid" or N <= SPLIT_SPAN:
        span = rng.randint(WIDE_SPAN + 1, min(SPLIT_SPAN, N))
    else:
        span = rng.randint(SPLIT_SPAN + 1, N)
    lo = rng.randint(0, N - span)
    inner = list(range(lo + 1, lo + span - 1))
    most = min(maxM, span) - 2
    if span == 1:
        return [lo]
    k = most if kind == "full" else rng.randint(0, min(most, 3)) if kind == "sparse" else rng.randint(0, most)
    sl = sorted([lo, lo + span - 1] + rng.sample(inner, k))
    if kind == "unordered":
        rng.shuffle(sl)
    return sl


def random_batches(N, rng):
    """N_RANDOM valid batches at window size N, each with its profile: what most of its tracks are."""
    out = []
    maxM = min(N, 40)
    for i in range(N_RANDOM):
        F = rng.randint(1, 60)
        profile = rng.choice(("mixed", "mixed", "ordered", "mid", "some_mid"))
        kinds = {"mixed": ("short", "mid", "long", "sparse", "full", "unordered"), "ordered": ("short", "mid", "long", "sparse", "full"),
                 "mid": ("mid", "mid", "mid", "short"), "some_mid": ("short", "short", "mid")}[profile]
        trk = [random_track(rng, N, maxM, rng.choice(kinds)) for _ in range(F)]
        vp = np.concatenate([[0], np.cumsum([len(t) for t in trk])])
        sl = [s for t in trk for s in t]
        b = batch(N, vp, sl, maxM=maxM, split=rng.random() < 0.85 and N > WIDE_SPAN, direct_cap=rng.choice((3840, 3840, 60, 16384)),
                  rem=rng.choice((-1, -1, -1, 96, 6)), rec_cap=-1 if rng.random() < 0.9 else F + rng.randint(0, 2), nch=rng.choice((1, 2, 5)))
        b["profile"] = profile
        out.append(b)
    return out
