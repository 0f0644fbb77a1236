"""The host's intake of a batch (`csrc/batch_order.h`: the per-track rules, `scan_range`, `BatchOrder::build`, the two byte
layouts) against `batch_order_model.py`, which restates it with lists and sorts.  `batch_order_driver.cpp` is built with the
host compiler from the header alone, reads batches as text and prints the scan's code, the keys and every field of the result;
the model's text must equal it.

1  shapes that occur: the five BASELINE configurations, the golden edge_* batches with long or ragged tracks, the two
   tests/regress batches; each with the split on and off
2  seeded random batches at N in {11, 12, 16, 31, 37, 65}; every branch of the intake is met (counted by the model)
3  invalid input: each error alone, the lowest range and the first view decide; a failed scan leaves the BatchOrder of the last
   good batch UNCHANGED (the scan never touches it), a failed build() leaves it INVALID (`valid` is cleared first, set last)
4  the layouts: alignment, no overlap, room for every record
5  tests/data/batch_order_parent.txt: one SHA-256 digest per batch of 1 and 2 from the loop bodies of msckf_set_features as
   they were before they had a header of their own

MSCKF_BATCH_ORDER_SCRIPTS=<directory> writes the scripts there (for a run of the driver built with sanitizers)."""
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from batch_order_model import (ERR_ARG, ERR_DUP_SLOT, N_RANDOM, OK, RANDOM_N, Order, batch, batch_lines, random_batches, text)
from msckf_amd import synth

HEADER_DIR = os.path.join(ROOT, "monocular-visual-inertial-msckf_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "batch_order_driver.cpp")
PARENT = os.path.join(ROOT, "tests", "data", "batch_order_parent.txt")
EDGES = ("edge_long_tracks", "edge_mixed_spans", "edge_few_long_among_short", "edge_few_rows_long_tracks", "edge_variable_tracks")
REGRESS = ("few_rows_wide_tracks_283", "few_rows_wide_tracks_373")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("batch_order"), "driver")
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, "-o", exe, DRIVER], check=True, timeout=120)

    def run(name, batches):
        """The driver's output, one block of lines per batch."""
        inp = "\n".join(text(b) for b in batches) + "\n"
        keep = os.environ.get("MSCKF_BATCH_ORDER_SCRIPTS")
        if keep:
            with open(os.path.join(keep, name + ".txt"), "w") as f:
                f.write(inp)
        out = subprocess.run([exe], input=inp, check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
        blocks, cur = [], []
        for line in out:
            cur.append(line)
            if line == "end":
                blocks.append(cur)
                cur = []
        assert not cur and len(blocks) == len(batches)
        return blocks
    return run


def replay(batches, blocks, seen=None):
    """The model, batch by batch, against the driver's blocks."""
    order = Order()
    for k, (b, got) in enumerate(zip(batches, blocks)):
        want = batch_lines(b, order, seen)
        assert got == want, (k, [(x, y) for x, y in zip(got, want) if x != y][:1], len(got), len(want))


# ---- the scripts ------------------------------------------------------------------------------------------------------------
def occurring():
    """[(name, batch)] of case 1."""
    probs = [(name, synth.make_problem(*synth.CONFIGS[name], seed=0)) for name in ("cfg1", "cfg2", "cfg3", "cfg4", "cfg5")]
    probs += [(name, load_golden(name)[0]) for name in EDGES]
    for name in REGRESS:
        d = np.load(os.path.join(ROOT, "tests", "regress", name + ".npz"))
        probs.append((name, synth.UpdateProblem(**{k: d[k] for k in d.files})))
    out = []
    for name, p in probs:
        for split in (1, 0):
            # (as the library scans them: on the host pool from 4096 tracks on)
            out.append((name, batch(p.N, p.view_ptr, np.asarray(p.obs_slot).reshape(-1), maxM=31, split=split, nch=8 if p.F >= 4096 else 1)))
    return out


def random_script(N):
    return random_batches(N, random.Random(1000 + N))


@pytest.fixture(scope="module")
def scripts(driver):
    """{name: (batches, the driver's blocks)} of cases 1 and 2, run once."""
    out = {"occurring": [b for _, b in occurring()]}
    for N in RANDOM_N:
        out["random_%d" % N] = random_script(N)
    return {name: (batches, driver(name, batches)) for name, batches in out.items()}


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_shapes_that_occur(scripts):
    batches, blocks = scripts["occurring"]
    seen = {}
    replay(batches, blocks, seen)
    assert all(b[0] == "rc 0" and b[3] == "build 0" for b in blocks)
    names = [name for name, _ in occurring()]
    split_on = {name: int(b[4].split()[12]) for name, b, bb in zip(names, blocks, batches) if bb["split"]}
    # configs[4] (every track 15 slots) keeps the 90-column tiles; the long-track fixtures are split; nothing is with the split off
    assert split_on["cfg5"] == 0 and blocks[names.index("cfg5")][1].endswith("keep 1")
    assert split_on["edge_long_tracks"] == 1 and split_on["few_rows_wide_tracks_283"] == 1 and split_on["cfg3"] == 0
    assert all(int(b[4].split()[12]) == 0 for b, bb in zip(blocks, batches) if not bb["split"])
    assert seen["class 2"] > 0 and seen["override: most tracks"] > 0


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
BRANCHES = ("class 2", "unsplittable long", "override: only most tracks", "override: only too many rows", "empty stretch",
            "one-view group", "N > 64", "record capacity", "remainder capacity")


def test_random_batches_meet_every_branch(scripts):
    seen = {}
    for N in RANDOM_N:
        batches, blocks = scripts["random_%d" % N]
        assert len(batches) == N_RANDOM
        mine = {}
        replay(batches, blocks, mine)
        for k, v in mine.items():
            seen[k] = seen.get(k, 0) + v
    for name in BRANCHES:
        assert seen.get(name, 0) > 0, (name, seen)
    # tracks of more than 31 views and tracks over more than SPLIT_MAXG groups' worth of slots were among them
    tr = [b["obs_slot"][a:c] for N in RANDOM_N for b in scripts["random_%d" % N][0] for a, c in zip(b["view_ptr"], b["view_ptr"][1:])]
    assert any(len(t) > 31 for t in tr) and any(max(t) - min(t) + 1 > 60 and t == sorted(t) for t in tr)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def good(N, seed, F=20):
    """A valid batch of F ordered tracks of 4+ views, scanned in one range."""
    rng = random.Random(seed)
    trk = [sorted(rng.sample(range(N), rng.randint(4, min(N, 12)))) for _ in range(F)]
    return batch(N, np.concatenate([[0], np.cumsum([len(t) for t in trk])]), [s for t in trk for s in t], maxM=12)


def spoil(b, f, what, view=1):
    """Batch b with one error in track f, at position `view` of it."""
    b = dict(b, view_ptr=list(b["view_ptr"]), obs_slot=list(b["obs_slot"]))
    a = b["view_ptr"][f]
    if what == "M < 1":                     # (an empty track: the offsets stay within the arrays)
        n = b["view_ptr"][f + 1] - a
        del b["obs_slot"][a:a + n]
        b["view_ptr"][f + 1:] = [x - n for x in b["view_ptr"][f + 1:]]
    elif what == "M > maxM":
        b["maxM"] = b["view_ptr"][f + 1] - a - 1
    elif what == "slot < 0":
        b["obs_slot"][a + view] = -1
    elif what == "slot >= N":
        b["obs_slot"][a + view] = b["N"]
    elif what == "duplicate":
        b["obs_slot"][a + view] = b["obs_slot"][a + view - 1]
    return b


CODES = {"M < 1": ERR_ARG, "M > maxM": ERR_ARG, "slot < 0": ERR_ARG, "slot >= N": ERR_ARG, "duplicate": ERR_DUP_SLOT}


@pytest.mark.parametrize("N", (30, 65))
def test_invalid_input(driver, N):
    base = good(N, seed=N)
    longest = max(range(20), key=lambda f: base["view_ptr"][f + 1] - base["view_ptr"][f])
    script, want = [base], [OK]
    for what, code in CODES.items():        # each error alone
        script.append(spoil(base, longest if what == "M > maxM" else 7, what))
        want.append(code)
    for nch in (1, 2, 5):                   # two different errors in different ranges (tracks 3 and 17): the lowest range decides
        script.append(dict(spoil(spoil(base, 17, "slot >= N"), 3, "duplicate"), nch=nch))
        want.append(ERR_DUP_SLOT)
        script.append(dict(spoil(spoil(base, 17, "duplicate"), 3, "slot >= N"), nch=nch))
        want.append(ERR_ARG)
    # two errors in one track: the first in view order decides
    script.append(spoil(spoil(base, 5, "duplicate", view=1), 5, "slot >= N", view=2))
    want.append(ERR_DUP_SLOT)
    script.append(spoil(spoil(base, 5, "slot >= N", view=1), 5, "duplicate", view=3))      # (view 3 repeats view 2)
    want.append(ERR_ARG)
    # a build() that fails, then a failing scan behind it, then the good batch again
    script += [dict(base, rec_cap=19), spoil(base, 7, "duplicate"), base]
    want += [OK, ERR_DUP_SLOT, OK]
    blocks = driver("invalid_%d" % N, script)
    replay(script, blocks)
    assert [b[0] for b in blocks] == ["rc %d" % c for c in want]
    first = blocks[0][4:blocks[0].index(next(x for x in blocks[0] if x.startswith("rec ")))]
    assert first[0].startswith("order Fb ")
    for b in blocks[1:-3]:
        assert b[1:-1] == first             # a failed scan: the last good batch's BatchOrder, field by field
    assert blocks[-3][3:] == ["build 1", "order invalid", "end"]
    assert blocks[-2][1:] == ["order invalid", "end"]
    assert blocks[-1] == blocks[0]


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def nums(line):
    return [int(x) for x in line.split() if x.lstrip("-").isdigit()]


def test_layouts(scripts):
    n = 0
    for name, (batches, blocks) in scripts.items():
        for b, blk in zip(batches, blocks):
            if blk[3] != "build 0":
                continue
            F, sum_m = len(b["view_ptr"]) - 1, b["view_ptr"][-1]
            head = nums(blk[4])
            Fb, Fw, Fs, n_narrow, sum_ms = head[:5]
            raw, so = nums(blk[-3]), nums(blk[-2])
            r_uv, r_base, r_m, r_rho, r_slot, raw_bytes, rec_cap, pin, split_off = raw
            assert r_base % 16 == 0 and raw_bytes % 16 == 0 and all(x % 8 == 0 for x in raw[:5] + [split_off])
            # [uv | base | m | rho | slot] | records | split records, none into the next
            ends = [r_uv + 16 * sum_m, r_base + 24 * F, r_m + 24 * F, r_rho + 8 * F, r_slot + 4 * sum_m, raw_bytes + 24 * Fs, split_off + 40 * Fw]
            assert all(e <= s for e, s in zip(ends, [r_base, r_m, r_rho, r_slot, raw_bytes, split_off, pin]))
            assert rec_cap >= F + n_narrow + Fw == Fs and raw_bytes + 24 * rec_cap + 40 * (F + 1) == pin
            o, feat_bytes = so[:10], so[10]
            assert o[9] % 16 == 0 and all(x % 8 == 0 for x in o)
            sizes = [16 * sum_ms, 24 * Fs, 24 * Fs, 8 * Fs, 8 * Fs, 4 * (Fs + 1), 4 * Fs, 4 * sum_ms, 4 * Fs, 32 * Fs]
            assert all(a + s <= nxt for a, s, nxt in zip(o, sizes, o[1:] + [feat_bytes]))
            n += 1
    assert n > 250


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def digests(blocks):
    return [hashlib.sha256("\n".join(b).encode()).hexdigest() for b in blocks]


def test_the_intake_gives_what_it_gave_before_the_move(scripts):
    with open(PARENT) as f:
        want = f.read().split()
    for name in ["occurring"] + ["random_%d" % N for N in RANDOM_N]:
        batches, blocks = scripts[name]
        got = [name, str(len(blocks))] + digests(blocks)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a == b, (name, "batch", k - 2)
        want = want[len(got):]
    assert not want
