"""The host's sweep schedules and tables (`csrc/sweep_plan.h`: `sweep_schedule`, `sweep_flush_table`, `sweep_gate_table`,
`sweep_publish_table`, the memo behind `sweep_tables`, and `sweep_root`, which builds a plan's root with the tables of the
merge level that rides in its launch) against `sweep_plan_model.py`, which states what the kernels rely on.
`sweep_plan_driver.cpp` is built with the host compiler from the header alone, reads nodes as text and prints their schedules
and tables; the model's text must equal it, the gate table's placement is checked against the fetch rule.

1  plan shapes that occur: roots of N in {2, 11, 30, 37, 53}, merge nodes of 2 .. 16 equal triangles, 90-column nodes
2  three seeded random scripts; both ring verdicts occur at rc = 4 and rc = 16, requirements are moved to earlier steps
3  the memo: hits, misses on every field of the key, replacement of the oldest entry, clearing
4  sweep_root: the image's layout, shared tables, the root read through the image
5  tests/data/sweep_tables_parent.txt: the output of 1 and 2 from the four table functions as they were before they had a header
   of their own, one digest per eight nodes (the text itself is 2 MB)

MSCKF_SWEEP_PLAN_SCRIPTS=<directory> writes the scripts there (for a run of the driver built with sanitizers)."""
import hashlib
import os
import random
import subprocess

import pytest

from conftest import ROOT
from sweep_plan_model import MEMO_CAP, Memo, node_lines, schedule

HEADER_DIR = os.path.join(ROOT, "monocular-visual-inertial-msckf_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "sweep_plan_driver.cpp")
PARENT = os.path.join(ROOT, "tests", "data", "sweep_tables_parent.txt")
SEEDS, N_RANDOM = (1, 2, 3), 300


def node(wtot, nf, adopt, gate, rc, folds):
    return dict(wtot=wtot, nf=nf, adopt=int(adopt), gate=int(gate), rc=rc, folds=[tuple(f) for f in folds])


def text(n):
    head = "node %d %d %d %d %d %d" % (n["wtot"], n["nf"], n["adopt"], n["gate"], n["rc"], len(n["folds"]))
    return " ".join([head] + ["%d %d %d %d %d" % f for f in n["folds"]])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("sweep_plan"), "driver")
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, "-o", exe, DRIVER], check=True, timeout=120)

    def run(name, script):
        """The driver's output, one block of lines per script line."""
        inp = "\n".join(script) + "\n"
        keep = os.environ.get("MSCKF_SWEEP_PLAN_SCRIPTS")
        if keep:
            with open(os.path.join(keep, name + ".txt"), "w") as f:
                f.write(inp)
        out = subprocess.run([exe], input=inp, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
        blocks, cur = [], []
        for line in out:
            cur.append(line)
            if line == "end":
                blocks.append(cur)
                cur = []
        assert not cur and len(blocks) == len(script)
        return blocks
    return run


def replay(nodes, blocks, memo=None):
    """The model, node by node, against the driver's blocks.  Returns (requirements moved, ring verdicts)."""
    memo = memo or Memo()
    moved, verdicts = 0, []
    for k, (n, got) in enumerate(zip(nodes, blocks)):
        want, m, ok = node_lines(n, got, memo)
        assert got == want, (k, text(n), [(a, b) for a, b in zip(got, want) if a != b][:1])
        moved += m
        verdicts.append(ok)
    return moved, verdicts


# ---- the shapes -----------------------------------------------------------------------------------------------------------
def root_folds(N, span, streamed, thin):
    """One group per first slot with a window of min(span, N - s) slots, every third missing where `thin`."""
    folds, env = [], 0
    for s in range(N):
        if thin and s % 3 == 2:
            continue
        w = 6 * min(span, N - s)
        env = max(env, 6 * s + w)
        folds.append((6 * s, w, env - 6 * s, len(folds) + 1 if streamed else 0, 64 if streamed else 0))
    return folds


def occurring():
    """[(name, node)] of case 1."""
    out = []
    for N in (2, 11, 30, 37, 53):
        for adopt in (1, 0):
            for streamed in (0, 1):
                for thin in (0, 1):
                    out.append(("root", node(6 * N, 8, adopt, streamed, 256, root_folds(N, 10, streamed, thin))))
    for k in range(2, 17):
        for nf in (8, 11, 12):
            for adopt in (1, 0):
                for prod in (0, 1):
                    folds = [(0, 60, 60, j + 1 if prod else 0, 64 if prod else 0) for j in range(k)]
                    out.append(("merge", node(60, nf, adopt, prod, 256, folds)))
    for N in (16, 40):                      # the ring form's 90-column tiles: windows of up to 15 slots, a ring of 128 rows
        for thin in (0, 1):
            out.append(("root90", node(6 * N, 8, 1, 0, 128, root_folds(N, 15, 0, thin))))
    for k in (2, 9, 16):
        out.append(("merge90", node(90, 8, 1, 0, 128, [(0, 90, 90, 0, 0)] * k)))
    return out


def random_nodes(seed):
    """1 to 30 folds on nf in {8, 11, 12} slots: root-like (offsets growing by 6, 12 or 18) or merge-like (all 0), widths
    6 {1 .. 10}, the envelope clipped at 60, a producer on three folds in four; small rings among the rc."""
    rng = random.Random(seed)
    out = []
    for _ in range(N_RANDOM):
        k, nf, rooty = rng.randint(1, 30), rng.choice((8, 11, 12)), rng.random() < 0.5
        folds, off, env = [], 0, 0
        for j in range(k):
            if rooty and j:
                off += rng.choice((6, 12, 18))
            w = 6 * rng.randint(1, 10)
            env = max(env, off + w)
            ew = min(env - off, 60)
            folds.append((off, w, ew, j + 1 if rng.random() < 0.75 else 0, rng.choice((0, 64))))
        wtot = max(f[0] + f[2] for f in folds)
        rc = rng.choice((4, 4, 4, 16, 16, 16, 64, 128, 256))
        out.append(node(wtot, nf, rng.random() < 0.5, rng.random() < 0.5, rc, folds))
    return out


# ---- 1 --------------------------------------------------------------------------------------------------------------------
def test_plan_shapes_that_occur(driver):
    cases = occurring()
    nodes = [n for _, n in cases]
    blocks = driver("occurring", [text(n) for n in nodes])
    moved, verdicts = replay(nodes, blocks)
    assert all(verdicts)                    # (what the planner makes fits its rings)
    assert moved > 0
    # the streamed roots' and the gated merges' requirements are there at all
    assert all(int(b[3].split()[1]) > 0 for (name, n), b in zip(cases, blocks) if n["gate"])
    # the kernels' header comment: t0[0] = 0, t0[1] = 1, then lag 7 between group triangles 6 columns apart, lag 1 in a merge
    assert cases[16][0] == "root" and nodes[16]["adopt"] == 1 and schedule(nodes[16])[0][:8] == [0, 1, 8, 15, 22, 29, 36, 43]
    assert schedule(node(60, 8, 1, 0, 256, [(0, 60, 60, 0, 0)] * 4)) == ([0, 1, 2, 3], 63)


# ---- 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_random_scripts(driver, seed):
    nodes = random_nodes(seed)
    blocks = driver("random_%d" % seed, [text(n) for n in nodes])
    moved, verdicts = replay(nodes, blocks)
    assert moved > 0
    for rc in (4, 16):
        assert {ok for n, ok in zip(nodes, verdicts) if n["rc"] == rc} == {True, False}, rc
    assert all(ok for n, ok in zip(nodes, verdicts) if n["rc"] >= 64)


# ---- 3 --------------------------------------------------------------------------------------------------------------------
def tables(block):
    """What a block says about the node itself: everything but the memo's slot and verdict."""
    return [line for line in block if not line.startswith("memo ")]


def test_the_memo(driver):
    base = node(72, 8, 1, 1, 256, [(0, 60, 60, 1, 64), (6, 60, 60, 2, 64), (12, 60, 60, 3, 64)])
    near = [dict(base, wtot=78), dict(base, nf=11), dict(base, adopt=0), dict(base, gate=0)]
    for i, bump in enumerate((6, 6, 6, 1, 1)):     # ... and every field of a fold
        f = list(base["folds"][2])
        f[i] = f[i] - bump if i == 1 else f[i] + bump
        near.append(dict(base, folds=base["folds"][:2] + [tuple(f)]))
    many = [node(60, 8, 1, 0, 256, [(0, 6 * (1 + j % 10), 60, 0, 0)] * (2 + j // 10)) for j in range(MEMO_CAP + 1)]
    nodes = [base, base] + near + [base] + many + [many[1], many[0], many[2]]
    script = [text(n) for n in nodes]
    blocks = driver("memo", script + ["clear"] + script)
    memo = Memo()
    replay(nodes, blocks[:len(nodes)], memo)
    memo.clear()
    assert blocks[len(nodes)] == ["end"]
    replay(nodes, blocks[len(nodes) + 1:], memo)
    verdict = [b[5] for b in blocks[:len(nodes)]]
    # a hit is the entry a rebuild gives; a key that differs in one field misses
    assert verdict[:2] == ["memo 0 0", "memo 0 1"] and tables(blocks[0]) == tables(blocks[1])
    assert verdict[2:2 + len(near)] == ["memo %d 0" % (1 + i) for i in range(len(near))]
    assert verdict[2 + len(near)] == "memo 0 1"
    # 65 more distinct keys fill the memo and then replace the oldest entries: slot 0 (base), slot 1, ...
    at = 3 + len(near)
    used = 1 + len(near)
    assert verdict[at:at + MEMO_CAP - used] == ["memo %d 0" % s for s in range(used, MEMO_CAP)]
    assert verdict[at + MEMO_CAP - used:at + len(many)] == ["memo %d 0" % s for s in range(used + 1)]
    tail = at + len(many)
    assert verdict[tail] == "memo %d 1" % (used + 1)                     # many[1] is still there
    assert verdict[tail + 1] == "memo %d 0" % (used + 1)                 # many[0] was the oldest of `many`... replaced, rebuilt
    assert tables(blocks[tail + 1]) == tables(blocks[at])
    assert verdict[tail + 2] == "memo %d 1" % (used + 2)
    # clearing the memo changes no output
    assert [tables(b) for b in blocks[len(nodes) + 1:]] == [tables(b) for b in blocks[:len(nodes)]]


# ---- 4 --------------------------------------------------------------------------------------------------------------------
def ints(line):
    return [int(x) for x in line.split()[1:] if x.lstrip("-").isdigit()]


@pytest.mark.parametrize("gated", (0, 1))
@pytest.mark.parametrize("N", (2, 11, 30, 37, 53))
def test_the_root_with_its_riding_level(driver, N, gated):
    ride_nf, dc = (8 if gated else 11), 6 * N
    # every third group is a single leaf (no producer); the others have a merge node of 2 + s % 3 triangles of their width
    tris, rides = [], []
    for s in range(N):
        w = 6 * min(10, N - s)
        if s % 3 == 2:
            tris.append((s, w, 0, 0))
            continue
        k = 2 + s % 3 + (s == 0) * 9        # (one node of more triangles than fold slots)
        rides.append(node(w, ride_nf, not gated, gated, 1 << 29, [(0, w, w, j + 1 if gated else 0, 64 if gated else 0) for j in range(k)]))
        tris.append((s, w, 64, len(rides)))
    if gated:
        rides[0]["folds"] = rides[0]["folds"][:8]

    def root_line(form, streamed, with_ride):
        parts = ["root %d %d %d %d %d %d %d" % (dc, form, streamed, len(tris), len(rides) if with_ride else 0, ride_nf, gated)]
        parts += ["%d %d %d %d" % t for t in tris]
        if with_ride:
            parts += ["%d %d " % (n["wtot"], len(n["folds"])) + " ".join("%d %d %d %d %d" % f for f in n["folds"]) for n in rides]
        return " ".join(parts)

    def as_node(streamed):
        folds, env = [], 0
        for s, w, ld, prod in tris:
            env = max(env, 6 * s + w)
            folds.append((6 * s, w, env - 6 * s, prod if streamed else 0, ld))
        return node(dc, 8, not streamed, streamed, 1 << 29, folds)

    singles = [as_node(1), as_node(0)] + rides
    script = [root_line(1, 1, True), root_line(1, 0, True), root_line(0, 0, False), "clear"] + [text(n) for n in singles]
    blocks = driver("root_%d_%d" % (N, gated), script)
    del blocks[3]
    replay(singles, blocks[3:])
    single = [dict(t0=ints(b[0]), nsteps=ints(b[1])[0], tab=ints(b[6][b[6].index(":"):]), n_gate=ints(b[6])[1]) for b in blocks[3:]]

    def parse(block, n_tri):
        head = block[0].split()
        out = dict(fold_begin=int(head[1]), fold_end=int(head[2]), wtot=int(head[3]), nsteps=int(head[4]), band=int(head[6]),
                   n_gate=int(head[8]), merge_at=int(head[10]), streamed=int(head[12]))
        out["folds"] = [tuple(ints(line)) for line in block[1:1 + n_tri]]
        out["rides"] = [ints(line) for line in block[1 + n_tri:-2]]
        out["image"] = ints(block[-2])
        assert block[-2].startswith("image") and block[-1] == "end"
        return out

    n_fold = sum(len(n["folds"]) for n in rides)
    # streamed: [root flush | root gate | n offsets | node tables]
    r, want = parse(blocks[0], len(tris)), single[0]
    assert (r["fold_begin"], r["fold_end"], r["wtot"], r["nsteps"]) == (n_fold, n_fold + len(tris), dc, want["nsteps"])
    assert [(f[0], f[1], f[2], f[4], f[5]) for f in r["folds"]] == singles[0]["folds"] and [f[3] for f in r["folds"]] == want["t0"]
    assert r["band"] == max(f[2] for f in singles[0]["folds"]) and r["streamed"] == 1 and r["n_gate"] == want["n_gate"] >= 0
    image, at = r["image"], r["merge_at"]
    assert image[:at] == want["tab"] and at == len(want["tab"])
    seen, behind = {}, at + len(rides)
    for i, n in enumerate(rides):
        s = single[2 + i]
        assert r["rides"][i] == [s["nsteps"], s["n_gate"]] + s["t0"]
        assert (s["n_gate"] >= 0) == bool(gated)
        o = image[at + i]
        assert image[behind + o:behind + o + len(s["tab"])] == s["tab"]
        key = text(n)
        assert seen.setdefault(key, o) == o                                   # equal nodes share one table
    offsets = sorted(set(seen.values()))
    assert len(seen) < len(rides) or N <= 11           # (full windows of ten slots repeat from N = 12 on)
    sizes = {o: len(single[2 + [text(n) for n in rides].index(k)]["tab"]) for k, o in seen.items()}
    assert offsets[0] == 0 and all(b == a + sizes[a] for a, b in zip(offsets, offsets[1:]))   # first seen first, nothing between
    assert len(image) == behind + offsets[-1] + sizes[offsets[-1]]
    # not streamed: the root's flush table alone; not in k_sweep form: the schedule and no image
    r, want = parse(blocks[1], len(tris)), single[1]
    assert (r["nsteps"], r["n_gate"], r["merge_at"], r["streamed"], r["image"]) == (want["nsteps"], -1, 0, 0, want["tab"])
    assert [f[3] for f in r["folds"]] == want["t0"] and all(f[4] == 0 for f in r["folds"])
    r = parse(blocks[2], len(tris))
    assert (r["fold_begin"], r["nsteps"], r["n_gate"], r["image"]) == (0, want["nsteps"], -1, []) and [f[3] for f in r["folds"]] == want["t0"]


# ---- 5 --------------------------------------------------------------------------------------------------------------------
CHUNK = 8


def digests(blocks):
    """One per CHUNK nodes, of their t0, nsteps, flush, gate and publish lines: what the four table functions alone decide."""
    lines = ["\n".join(b[:5]) for b in blocks]
    return [hashlib.sha256("\n".join(lines[k:k + CHUNK]).encode()).hexdigest()[:16] for k in range(0, len(lines), CHUNK)]


def test_the_functions_give_what_they_gave_before_the_move(driver):
    scripts = [("occurring", [n for _, n in occurring()])] + [("random_%d" % s, random_nodes(s)) for s in SEEDS]
    with open(PARENT) as f:
        want = f.read().split()
    for name, nodes in scripts:
        got = [name, str(len(nodes))] + digests(driver(name, [text(n) for n in nodes]))
        for k, (a, b) in enumerate(zip(got, want)):
            assert a == b, (name, "nodes from", (k - 2) * CHUNK, [text(n) for n in nodes[(k - 2) * CHUNK:(k - 1) * CHUNK]])
        want = want[len(got):]
    assert not want
