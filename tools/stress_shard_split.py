#!/usr/bin/env python3
"""Sharded twin of stress_split.py: ragged long-track batches through split records (the calls of RcclShardedUpdate with S
logical shards on ONE engine, tests/test_gpu_shard_split.py) against the oracle, and bit for bit with the batch's first
result.  usage: stress_shard_split.py [rounds] [batches]"""
import importlib.util, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msckf_amd
from msckf_amd.api import UpdateEngine
from msckf_amd.shard import partition_features
from oracle import msckf_oracle as oracle
import test_gpu_shard_split as t
spec = importlib.util.spec_from_file_location("soak_holes", os.path.join(ROOT, "tools", "soak_holes.py"))
sh = importlib.util.module_from_spec(spec); spec.loader.exec_module(sh)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 24
rng = np.random.default_rng(13)
cases = []
while len(cases) < nb:
    N = int(rng.integers(11, 54)); F = int(rng.integers(20, 400))
    hi = int(rng.integers(11, min(N, 31) + 1))
    p = sh.ragged(rng, N, F, 2, hi, float(rng.choice([0.0, 0.1, 0.4])))
    shards = partition_features(p.view_ptr, int(rng.integers(2, 9)))
    from msckf_amd.api import exchange_split_rule
    if not exchange_split_rule(p, shards)["split"]:
        continue
    cases.append((p, shards, oracle.update(p, dense_noise=False)))
first = [None] * nb
bad = calls = 0
t0 = time.time()
with UpdateEngine(max_clones=53, max_features=400, max_track=31) as eng:
    for rd in range(rounds):
        for i, (p, shards, ref) in enumerate(cases):
            try:
                res = t._split_merge(eng, p, shards, ref, calls=1)
                calls += 1
                if first[i] is None:
                    first[i] = (res.dx, res.P_new)
                elif not (np.array_equal(res.dx, first[i][0]) and np.array_equal(res.P_new, first[i][1])):
                    raise AssertionError("not bit-identical with the first call")
            except AssertionError as e:
                bad += 1
                print("BAD round %d case %d (N %d, F %d, %d shards): %s" % (rd, i, p.N, p.F, len(shards), e), flush=True)
print("%d sharded calls (%d merges + their %d shard records), %d bad, %.0f s" %
      (calls, calls, sum(len(c[1]) for c in cases) * rounds, bad, time.time() - t0))
