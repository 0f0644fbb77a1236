"""Parity tests proper: the HIP path, called through the C-ABI, against
 (a) the golden fixtures captured from the reference,
 (b) the oracle on freshly seeded problems,
 (c) size-independent properties at BASELINE.json's full sizes.
Tolerance: 1e-8 relative on dx and P+ (BASELINE.json north_star); observed ~1e-14."""
import numpy as np
import pytest

import filter_prior as fp
from conftest import golden_cases, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.fixture(scope="module")
def eng():
    from msckf_amd.api import UpdateEngine
    e = UpdateEngine(max_clones=53, max_features=20000, max_track=31)
    yield e
    e.close()


@pytest.mark.parametrize("case", golden_cases())
def test_golden(eng, case):
    prob, ref = load_golden(case)
    res = eng.update_problem(prob)
    assert res.status == int(ref["status"])
    assert np.array_equal(res.accepted, ref["accepted"])
    assert res.n_rejected == int(ref["n_rejected"])
    gam, q = eng.debug_gate()
    np.testing.assert_allclose(gam, ref["gamma"], rtol=1e-9, atol=1e-12)
    assert rel_err(res.dx, ref["dx"]) < TOL
    assert rel_err(res.P_new, ref["P_new"]) < TOL
    assert np.array_equal(res.P_new, res.P_new.T)
    if case.endswith("_B") or case == "edge_gauge_prior":
        # priors whose sigmas span orders of magnitude: every entry in units of its own sigmas, and the update term by itself
        # (tests/filter_prior.py: what the Frobenius norm over the whole array cannot see there)
        s_dx, s_P, u_P = fp.metrics(res.dx, res.P_new, ref, prob.P)[2:]
        print(f"FILTERPRIOR golden_{case} scaled dx {s_dx:.2e} scaled P {s_P:.2e} update term {u_P:.2e}")
        assert s_dx < TOL and s_P < TOL and u_P < TOL, (s_dx, s_P, u_P)
    if res.status == 0:
        # basis-invariant check of the compressed system: T^T T = H^T H, T^T r_n = H^T r
        T, rn = eng.debug_compressed()
        d = prob.d
        G = np.zeros((d, d)); G[15:, 15:] = T.T @ T
        b = np.zeros(d); b[15:] = T.T @ rn
        assert rel_err(G, ref["G"]) < 1e-10
        assert rel_err(b, ref["b"]) < 1e-10
        assert np.allclose(np.tril(T, -1), 0.0)
        assert res.stats["stacked_rows"] == int(sum(q[res.accepted == 1]))
    else:
        assert np.array_equal(res.P_new, prob.P) and not res.dx.any()     # untouched state, MSCKF.py:584-585


@pytest.mark.parametrize("N,F,M,seed,kw", [
    (10, 50, 5, 21, {}),
    (20, 500, 8, 22, {"outlier_fraction": 0.1, "outlier_px": 500.0}),
    (12, 300, 12, 23, {"variable_tracks": True}),
    (31, 64, 31, 24, {}),                      # maximum track length, every row of the wavefront in use
    (50, 400, 15, 25, {}),                     # N = 50 (d = 315): S too large for the LDS Cholesky path
    (6, 3, 2, 26, {}),                         # two-view tracks: one projected row each
    (32, 200, 8, 27, {}),                      # dc = 192: just past one register-tiled Cholesky -> two-block K6 (160 + 32)
    (45, 300, 10, 28, {"outlier_fraction": 0.05, "outlier_px": 500.0}),   # two-block K6, 160 + 110
    (53, 200, 6, 29, {}),                      # dc = 318: the widest two-block window (160 + 158)
    (2, 6, 2, 30, {}),                         # dc = 12: one partly filled 16 x 16 block in the Cholesky
    (3, 12, 3, 33, {}),                        # dc = 18: two blocks, the second with two columns
    (10, 1, 5, 3, {}),                         # ONE feature: one leaf, one row block on the prefetched tile (round 3: the compiler
    (10, 2, 5, 3, {}),                         #   put a register copy in front of a lone DPP statement of the column step --
    (10, 6, 10, 3, {}),                        #   7.7e-6 on dx here, 1e-1 at 50 features; sweep_dpp_groups.h is the fix)
    (40, 300, 10, 1, {}),                      # ring-buffered sweep (N > 37) behind 60-column leaves
])
def test_against_oracle(eng, N, F, M, seed, kw):
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(N, F, M, seed=seed, **kw)
    ref = oracle.update(prob, dense_noise=False)
    res = eng.update_problem(prob)
    assert res.status == ref["status"]
    assert np.array_equal(res.accepted, ref["accepted"])
    assert rel_err(res.dx, ref["dx"]) < TOL
    assert rel_err(res.P_new, ref["P_new"]) < TOL


def test_resident_path_equals_one_shot(eng):
    prob, ref = load_golden("cfg2_A")
    one = eng.update_problem(prob)
    eng.load(prob)
    eng.run()
    r1 = eng.result()
    eng.run()                                   # same inputs again: bitwise reproducible
    r2 = eng.result()
    assert np.array_equal(r1.dx, one.dx) and np.array_equal(r1.P_new, one.P_new)
    assert np.array_equal(r1.dx, r2.dx) and np.array_equal(r1.P_new, r2.P_new)
    ms, stages = eng.run_timed(5, stages=True)
    assert ms > 0 and len(stages) == 3 and all(s > 0 for s in stages)


def test_bitwise_repeatability_stress(eng):
    """Race screen: the same update 25 times must give bit-identical dx / P+ (the kernels
    hand data between wavefronts through LDS with one barrier per eliminated column)."""
    for case in ("cfg2_A", "cfg3_A", "edge_variable_tracks"):
        prob, ref = load_golden(case)
        eng.load(prob)
        eng.run()
        first = eng.result()
        assert rel_err(first.dx, ref["dx"]) < TOL
        for _ in range(24):
            eng.run()
            r = eng.result()
            assert np.array_equal(r.dx, first.dx) and np.array_equal(r.P_new, first.P_new)


def test_feature_order_invariance_full_size(eng):
    """Headline size (N=30, F=2000, M=10): dx and P+ do not depend on the order of
    the feature dict nor on the QR tree shape."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    prob = synth.make_problem(30, 2000, 10, seed=5)
    base = eng.update_problem(prob)
    assert base.status == 0
    rng = np.random.default_rng(0)
    perm = rng.permutation(prob.F)
    M = 10
    idx = (perm[:, None] * M + np.arange(M)[None, :]).reshape(-1)
    p2 = synth.UpdateProblem(P=prob.P, cam_R=prob.cam_R, cam_t=prob.cam_t, cam_R0=prob.cam_R0, cam_t0=prob.cam_t0,
                             gravity=prob.gravity, K=prob.K, sigma=prob.sigma, view_ptr=prob.view_ptr,
                             obs_uv=prob.obs_uv[idx], obs_slot=prob.obs_slot[idx], idp_base=prob.idp_base[perm],
                             idp_m=prob.idp_m[perm], idp_rho=prob.idp_rho[perm])
    r2 = eng.update_problem(p2)
    assert np.array_equal(r2.accepted, base.accepted[perm])
    assert rel_err(r2.dx, base.dx) < 1e-10 and rel_err(r2.P_new, base.P_new) < 1e-11
    with UpdateEngine(max_clones=30, max_features=2000, max_track=10, leaf_rows=400, merge_arity=2) as e3:
        r3 = e3.update_problem(prob)
    assert rel_err(r3.dx, base.dx) < 1e-10 and rel_err(r3.P_new, base.P_new) < 1e-11


def test_covariance_properties_full_size(eng):
    """cfg3-size update: P+ symmetric, P - P+ positive semidefinite (information
    only adds), and the update is the oracle's (checked through the fixture)."""
    prob, ref = load_golden("cfg3_A")
    res = eng.update_problem(prob)
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
    ev = np.linalg.eigvalsh(prob.P - res.P_new)
    assert ev.min() > -1e-12 * abs(ev).max()
    assert np.linalg.eigvalsh(res.P_new).min() > 0


@pytest.mark.parametrize("case", ["cfg1_B", "cfg2_B"])
def test_recipe_b_spectrum_matches_the_reference(eng, case):
    """Recipe B: covariance and poses produced by the reference's own process_imu / state_augmentation, cond(P) ~ 1e18,
    smallest eigenvalue a rounding-level negative.  The update here is the sequential block form P+ = P - sum_I X_I X_I^T
    (csrc/k_gstream.h), the reference's the Joseph form (MSCKF.py:613): the whole SPECTRUM of P+ must agree with the
    reference fixture's, the smallest eigenvalue included, to 1e-12 of the largest one, and P - P+ must be positive
    semidefinite to the same level (an update only removes uncertainty)."""
    prob, ref = load_golden(case)
    res = eng.update_problem(prob)
    assert res.status == 0
    assert np.array_equal(res.P_new, res.P_new.T)
    ev, ev_ref = np.linalg.eigvalsh(res.P_new), np.linalg.eigvalsh(ref["P_new"])
    scale = abs(ev_ref).max()
    assert abs(ev - ev_ref).max() < 1e-12 * scale, (ev[0], ev_ref[0], scale)
    assert abs(ev[0] - ev_ref[0]) < 1e-12 * scale
    gain = np.linalg.eigvalsh(prob.P - res.P_new)
    assert gain.min() > -1e-12 * abs(np.linalg.eigvalsh(prob.P)).max()


def test_malformed_view_ptr_in_a_large_batch(eng):
    """The CSR offsets of a batch large enough for the host worker pool (>= 1024 features) are checked as a whole BEFORE
    any feature range reads obs_slot through them: a non-monotone or wild view_ptr returns MSCKF_ERR_ARG (round-3 advisor:
    the parallel validation could read far outside obs_slot)."""
    from msckf_amd import synth
    from msckf_amd._ffi import EngineError, ERR_ARG
    good = synth.make_problem(12, 2048, 5, seed=71)
    for where, val in ((1500, -(2 ** 30)), (1500, 2 ** 30), (700, 3), (2048, 2 ** 30)):
        bad = synth.UpdateProblem(**{**good.__dict__})
        vp = good.view_ptr.copy(); vp[where] = val
        bad.view_ptr = vp
        with pytest.raises(EngineError) as ei:
            eng.load(bad)
        assert ei.value.code == ERR_ARG, (where, val)
    eng.load(good)                                           # and the engine recovers
    eng.run()
    assert eng.result().status == 0


@pytest.mark.parametrize("shards", [2, 3, 4])
def test_logical_shards_on_one_gpu(eng, shards):
    """Shard-merge invariance: S logical shards compressed
    one after the other on one GPU, merged, equal the single-shard update."""
    from msckf_amd.shard import partition_features
    prob, ref = load_golden("cfg2_B")
    blocks, total, acc = [], 0, np.zeros(prob.F, dtype=np.uint8)
    for lo, hi in partition_features(prob.view_ptr, shards):
        eng.load(prob.subset(lo, hi))
        eng.run_compress()
        blk, n = eng.export_block()
        acc[lo:hi] = eng.result().accepted
        blocks.append(blk); total += n
    eng.set_state(prob)
    eng.merge_gain(np.stack(blocks), total)
    res = eng.result()
    assert res.status == 0 and np.array_equal(acc, ref["accepted"])
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL


def test_sharded_driver_world1(eng):
    from msckf_amd.shard import HipShardBackend, ShardedUpdate
    prob, ref = load_golden("edge_some_rejected")
    status, dx, P_new, acc = ShardedUpdate(HipShardBackend(eng), 0, 1).update(prob)
    assert status == 0 and np.array_equal(acc, ref["accepted"])
    assert rel_err(dx, ref["dx"]) < TOL and rel_err(P_new, ref["P_new"]) < TOL


def test_two_consecutive_updates_keep_covariance_resident(eng):
    """P stays in HBM between updates: update, commit, update."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    p1 = synth.make_problem(15, 120, 6, seed=31)
    p2 = synth.make_problem(15, 100, 7, seed=32, poses=(p1.cam_R, p1.cam_t))   # same clones, new tracks
    o1 = oracle.update(p1)
    p2.P = o1["P_new"]
    o2 = oracle.update(p2)
    eng.load(p1); eng.run()
    assert eng.commit_covariance() == 0
    eng.set_features(p2); eng.run()
    r2 = eng.result()
    assert rel_err(r2.dx, o2["dx"]) < TOL and rel_err(r2.P_new, o2["P_new"]) < TOL


def test_reference_shaped_adapter(eng):
    """`UpdateEngine.update(filt, features)` mutates reference-shaped objects the
    way MSCKF.update + correct do (poses, biases, covariance, counter)."""
    from test_host_logic import make_reference_shaped
    prob, ref = load_golden("edge_some_rejected")
    filt, feats = make_reference_shaped(prob, ref)
    assert eng.update(filt, feats) == 0
    assert filt.number_of_residuals_discarded_for_gasting_test == int(ref["n_rejected"])
    assert rel_err(filt.state.covariance, ref["P_new"]) < TOL
    np.testing.assert_allclose(filt.state.imu.T_W_Ii.R, ref["post_imu_R"], atol=1e-9)
    np.testing.assert_allclose(filt.state.imu.T_W_Ii.t, ref["post_imu_t"], atol=1e-9)
    for i, cam in enumerate(filt.state.cameras.values()):
        np.testing.assert_allclose(cam.T_W_Ci.R, ref["post_cam_R"][i], atol=1e-9)
        np.testing.assert_allclose(cam.T_W_Ci.t, ref["post_cam_t"][i], atol=1e-9)


def test_error_codes(eng):
    from msckf_amd import _ffi, synth
    prob = synth.make_problem(8, 10, 4, seed=1)
    bad = synth.UpdateProblem(**{**prob.__dict__})
    bad.obs_slot = prob.obs_slot.copy(); bad.obs_slot[1] = bad.obs_slot[0]      # same clone twice in a track
    with pytest.raises(_ffi.EngineError) as e:
        eng.update_problem(bad)
    assert e.value.code == _ffi.ERR_DUP_SLOT
    bad2 = synth.UpdateProblem(**{**prob.__dict__})
    bad2.obs_slot = prob.obs_slot.copy(); bad2.obs_slot[0] = 99
    with pytest.raises(_ffi.EngineError) as e:
        eng.update_problem(bad2)
    assert e.value.code == _ffi.ERR_ARG
    empty = prob.subset(0, 0)
    res = eng.update_problem(empty)                                              # empty dict: no-op
    assert res.status == 1 and np.array_equal(res.P_new, prob.P)


def test_torch_shares_the_device():
    """torch (plumbing for the RCCL gather) and the engine in one process: export a block
    straight into a torch-owned HBM buffer and merge from it.  torch must be imported BEFORE
    the engine library is loaded (both bring a libamdhip64.so.7; the first one loaded serves
    the process), so this runs in a fresh interpreter."""
    import subprocess
    import sys
    from conftest import ROOT
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')
import torch
assert torch.cuda.is_available(), 'torch sees no GPU'
import msckf_amd
from msckf_amd.api import UpdateEngine
from conftest import load_golden, rel_err
prob, ref = load_golden('cfg1_A')
eng = UpdateEngine(max_clones=10, max_features=64, max_track=8)
eng.load(prob); eng.run_compress()
host_blk, n = eng.export_block()
buf = torch.zeros(eng.block_doubles(), dtype=torch.float64, device='cuda:0')
eng.export_block(dst_ptr=buf.data_ptr())
torch.cuda.synchronize()
assert np.array_equal(buf.cpu().numpy().reshape(host_blk.shape), host_blk)
eng.set_state(prob)
eng.merge_gain(int(buf.data_ptr()), n, n_blocks=1)
res = eng.result()
assert res.status == 0 and rel_err(res.dx, ref['dx']) < 1e-8 and rel_err(res.P_new, ref['P_new']) < 1e-8
out = torch.zeros(prob.d + prob.d ** 2, dtype=torch.float64, device='cuda:0')
eng.export_result(out.data_ptr(), out.data_ptr() + 8 * prob.d)
torch.cuda.synchronize()
assert np.array_equal(out[:prob.d].cpu().numpy(), res.dx)
# rank 0's broadcast buffer: the engine's own result range dx | P+ wrapped without a copy
view = torch.as_tensor(eng.result_device_view(), device='cuda')
assert view.shape == (prob.d + prob.d ** 2,)
assert np.array_equal(view[:prob.d].cpu().numpy(), res.dx)
assert np.array_equal(view[prob.d:].cpu().numpy().reshape(prob.d, prob.d), res.P_new)
# group exchange through HBM buffers: records exported without reading the gate back, counts taken from the records
from msckf_amd import synth
from msckf_amd.shard import partition_features as pf
from oracle import msckf_oracle as oracle
prob3 = synth.make_problem(20, 300, 8, seed=7)
ref3 = oracle.update(prob3, dense_noise=False)
eng3 = UpdateEngine(max_clones=20, max_features=300, max_track=8)
eng3.set_group_exchange(True)
shards = pf(prob3.view_ptr, 3)
bufs = None
for i, (lo, hi) in enumerate(shards):
    eng3.load(prob3.subset(lo, hi)); eng3.run_compress()
    if bufs is None:
        bufs = torch.zeros(3 * eng3.group_record_doubles(), dtype=torch.float64, device='cuda:0')
    _, n3 = eng3.export_groups(dst_ptr=bufs.data_ptr() + i * eng3.group_record_doubles() * 8, count=False)
    assert n3 == -1
torch.cuda.synchronize()
eng3.set_state(prob3)
eng3.merge_groups(int(bufs.data_ptr()), -1, n_records=3)
r3 = eng3.result()
assert r3.status == 0 and int(r3.stats['n_accepted']) == int(ref3['accepted'].sum())
assert rel_err(r3.dx, ref3['dx']) < 1e-8 and rel_err(r3.P_new, ref3['P_new']) < 1e-8
# the bench's N>1 data path with 3 shards on one device: blocks gathered in a torch HBM buffer
from msckf_amd.shard import partition_features
prob2, ref2 = load_golden('cfg2_B')
eng2 = UpdateEngine(max_clones=20, max_features=600, max_track=8)
nb = None; total = 0
parts = partition_features(prob2.view_ptr, 3)
gathered = None
for r, (lo, hi) in enumerate(parts):
    eng2.load(prob2.subset(lo, hi)); eng2.run_compress()
    if gathered is None:
        nb = eng2.block_doubles(); gathered = torch.zeros(3 * nb, dtype=torch.float64, device='cuda:0')
    _, n = eng2.export_block(dst_ptr=gathered.data_ptr() + 8 * nb * r); total += n
torch.cuda.synchronize()
eng2.set_state(prob2)
eng2.merge_gain(int(gathered.data_ptr()), total, n_blocks=3)
r2 = eng2.result()
assert r2.status == 0 and rel_err(r2.dx, ref2['dx']) < 1e-8 and rel_err(r2.P_new, ref2['P_new']) < 1e-8
print('TORCH_INTEROP_OK')
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "TORCH_INTEROP_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("N,F,M,seed,kw", [
    (30, 2000, 10, 31, {}),                                        # headline shape: 21 groups, 7 leaves each
    (20, 500, 8, 32, {"outlier_fraction": 0.1, "outlier_px": 500.0}),
    (12, 300, 10, 33, {"variable_tracks": True}),                  # ragged windows
    (30, 300, 10, 5, {"variable_tracks": True}),                   # ... with groups whose longest track is shorter than the
    (30, 120, 10, 6, {"variable_tracks": True}),                   #     reach of earlier groups: envelopes wider than the sources
    (10, 7, 3, 34, {}),                                            # fewer features than groups, single-row leaves
    (37, 600, 10, 35, {}),                                         # widest band R that still fits LDS next to the tiles
])
def test_band_pipeline_equals_merge_tree(N, F, M, seed, kw):
    """K5 through the band pipeline (per-group leaves, k_sweep group merges and root sweep) gives the
    update of the merge tree (k_fold levels) and of the oracle; T differs only by row signs / order."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(N, F, M, seed=seed, **kw)
    ref = oracle.update(prob, dense_noise=False)
    out = {}
    for plan in ("auto", "tree"):
        with UpdateEngine(max_clones=N, max_features=F, max_track=max(M, 2), plan=plan) as e:
            res = e.update_problem(prob)
            T, rn = e.debug_compressed()
            out[plan] = (res, T, rn)
    band, tree = out["auto"][0], out["tree"][0]
    assert band.status == tree.status == ref["status"] == 0
    assert np.array_equal(band.accepted, tree.accepted)
    assert rel_err(band.dx, tree.dx) < 1e-10 and rel_err(band.P_new, tree.P_new) < 1e-11
    assert rel_err(band.dx, ref["dx"]) < TOL and rel_err(band.P_new, ref["P_new"]) < TOL
    Tb, rb = out["auto"][1:]
    Tt, rt = out["tree"][1:]
    assert np.allclose(np.tril(Tb, -1), 0.0)
    assert rel_err(Tb.T @ Tb, Tt.T @ Tt) < 1e-11 and rel_err(Tb.T @ rb, Tt.T @ rt) < 1e-10
    # the band plan was taken: its R has no entry further than 6 * span columns right of the diagonal
    span = int((prob.obs_slot.reshape(-1)[np.asarray(prob.view_ptr[1:]) - 1]
                - prob.obs_slot.reshape(-1)[np.asarray(prob.view_ptr[:-1])]).max()) + 1
    assert not np.triu(Tb, 6 * span).any()


def _drop_views(prob, rng, keep_first=True, p_drop=0.35, only_first_slots=None):
    """Remove interior observations (tracks that skip clones) and, optionally, whole features so that only
    some first slots carry tracks (groups with gaps between them)."""
    from msckf_amd import synth
    vp = np.asarray(prob.view_ptr)
    keep_feat, new_vp, keep_obs = [], [0], []
    for f in range(prob.F):
        a, b = int(vp[f]), int(vp[f + 1])
        if only_first_slots is not None and int(prob.obs_slot[a]) not in only_first_slots:
            continue
        idx = [a] + [i for i in range(a + 1, b - 1) if rng.random() > p_drop] + [b - 1]
        idx = sorted(set(idx))
        if len(idx) < 2:
            continue
        keep_feat.append(f)
        keep_obs.extend(idx)
        new_vp.append(new_vp[-1] + len(idx))
    kf, ko = np.asarray(keep_feat), np.asarray(keep_obs)
    return synth.UpdateProblem(P=prob.P, cam_R=prob.cam_R, cam_t=prob.cam_t, cam_R0=prob.cam_R0, cam_t0=prob.cam_t0,
                               gravity=prob.gravity, K=prob.K, sigma=prob.sigma,
                               view_ptr=np.asarray(new_vp, dtype=np.int32), obs_uv=prob.obs_uv[ko],
                               obs_slot=prob.obs_slot[ko], idp_base=prob.idp_base[kf], idp_m=prob.idp_m[kf],
                               idp_rho=prob.idp_rho[kf])


@pytest.mark.parametrize("N,F,M,seed,kw,band", [
    (16, 120, 14, 36, {}, 90),                          # tracks of 11-15 slots: the 90-column sweep tiles (k_wsweep<6>)
    (50, 400, 15, 37, {}, 90),                          # ... with the band R in a ring of 128 rows (d = 315)
    (30, 500, 15, 38, {"variable_tracks": True}, 90),   # ragged tracks up to 15 slots
    (24, 300, 13, 39, {"outlier_fraction": 0.1, "outlier_px": 500.0}, 90),
    (52, 300, 10, 40, {}, 60),                          # 60-column tiles, 312 rows of R: ring of 256 rows (k_wsweep<4>)
    (31, 64, 31, 24, {}, None),                         # tracks wider than any sweep tile: split
])
def test_wide_sweep_and_ring(N, F, M, seed, kw, band):
    """Batches the plain sweep kernel cannot take -- tracks spanning 11-15 clone slots, band R larger than
    LDS -- run the general sweep (wider register tiles, R in a ring with a static flush schedule); beyond
    15 slots the merge tree.  All against the oracle; the band plan shows in the zero pattern of T."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(N, F, M, seed=seed, **kw)
    ref = oracle.update(prob, dense_noise=False)
    # (tracks of 11+ slots are split by default, DESIGN.md 3.6: plan="band" keeps them whole, on the
    #  90-column tiles this test is about; the default plan of the same batches is test_mixed_track_spans' subject)
    with UpdateEngine(max_clones=N, max_features=F, max_track=max(M, 2), plan="band" if band is not None else "auto") as e:
        res = e.update_problem(prob)
        assert res.status == ref["status"] == 0
        assert np.array_equal(res.accepted, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
        T, rn = e.debug_compressed()
        H, r = ref["H_X"][:, 15:], ref["r_o"]
        assert rel_err(T.T @ T, H.T @ H) < 1e-10 and rel_err(T.T @ rn, H.T @ r) < 1e-10
        assert np.allclose(np.tril(T, -1), 0.0)
        if band is not None:
            assert not np.triu(T, band).any()             # a band plan ran
            assert res.stats["n_levels"] >= 2
        e.load(prob)                                      # resident path, twice: bitwise reproducible
        e.run(); r1 = e.result()
        e.run(); r2 = e.result()
        assert np.array_equal(r1.dx, r2.dx) and np.array_equal(r1.P_new, r2.P_new)


def _concat_problems(a, b):
    from msckf_amd import synth
    vp = np.concatenate([a.view_ptr, a.view_ptr[-1] + b.view_ptr[1:]])
    cat = lambda x, y: np.concatenate([x, y])
    return synth.UpdateProblem(**{**a.__dict__, "view_ptr": vp.astype(np.int32), "obs_uv": cat(a.obs_uv, b.obs_uv),
                                  "obs_slot": cat(a.obs_slot, b.obs_slot), "idp_base": cat(a.idp_base, b.idp_base),
                                  "idp_m": cat(a.idp_m, b.idp_m), "idp_rho": cat(a.idp_rho, b.idp_rho)})


@pytest.mark.parametrize("N,F,M,seed,kw", [
    (30, 400, 30, 51, {"variable_tracks": True, "min_track": 2}),                 # tracks of 2 .. 30 slots: every class at once
    (30, 300, 30, 52, {"variable_tracks": True, "min_track": 2, "outlier_fraction": 0.15, "outlier_px": 300.0}),
    (24, 200, 24, 53, {"variable_tracks": True, "min_track": 12}),                # 90-column band tracks + wide ones
    (31, 120, 31, 54, {"variable_tracks": True, "min_track": 16}),                # wide tracks only, 6N + 1 = 187 columns
    (16, 80, 16, 55, {}),                                                         # the narrowest wide track: 16 slots
    (20, 150, 20, 56, {"variable_tracks": True, "min_track": 2}),
])
def test_mixed_track_spans(N, F, M, seed, kw):
    """The reference's window is 30 clones (MSCKF.py:45), a track grows one view per frame until it is lost (:404-412) and
    both pruning callers hand `update` every feature of the removed clones (:669-678, :726-735): a batch mixes spans.  Tracks
    of up to 10 slots take the band pipeline as they are, longer ones as the blocks of their split, K6-K7 takes both sources of rows.
    Against the oracle at the parity tolerance; bit-reproducible."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(N, F, M, seed=seed, **kw)
    ref = oracle.update(prob, dense_noise=False)
    with UpdateEngine(max_clones=N, max_features=F, max_track=max(M, 2)) as e:
        res = e.update_problem(prob)
        assert res.status == ref["status"] == 0
        assert np.array_equal(res.accepted, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
        assert np.array_equal(res.P_new, res.P_new.T)
        e.load(prob)
        e.run(); r1 = e.result()
        e.run(); r2 = e.result()
        assert np.array_equal(r1.dx, r2.dx) and np.array_equal(r1.P_new, r2.P_new)


def test_a_few_long_tracks_among_short_ones():
    """1990 ten-view tracks + 10 thirty-view tracks (the shape one long-lived feature gives a frame's batch): the long ones must
    not drag the batch out of the band pipeline.  Parity against the oracle on a smaller instance of the same shape, and the
    all-rejected corner of the wide class (its Gram matrix is then exactly zero)."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    a = synth.make_problem(30, 300, 10, seed=61)
    b = synth.make_problem(30, 6, 30, seed=62, P=a.P, poses=(a.cam_R, a.cam_t))
    prob = _concat_problems(a, b)
    ref = oracle.update(prob, dense_noise=False)
    with UpdateEngine(max_clones=30, max_features=400, max_track=30) as e:
        res = e.update_problem(prob)
        assert res.status == ref["status"] == 0
        assert np.array_equal(res.accepted, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
        # the wide tracks all rejected by the gate (gross outliers on every one of them): the band tracks alone update
        bad = synth.make_problem(30, 6, 30, seed=63, P=a.P, poses=(a.cam_R, a.cam_t), outlier_fraction=1.0, outlier_px=800.0)
        prob2 = _concat_problems(a, bad)
        ref2 = oracle.update(prob2, dense_noise=False)
        res2 = e.update_problem(prob2)
        assert res2.status == ref2["status"] == 0
        assert np.array_equal(res2.accepted, ref2["accepted"]) and not res2.accepted[300:].any()
        assert rel_err(res2.dx, ref2["dx"]) < TOL and rel_err(res2.P_new, ref2["P_new"]) < TOL


@pytest.mark.parametrize("seed,first_slots", [(44, None), (45, {0, 3, 20, 21}), (46, {11})])
def test_wide_sweep_tracks_with_holes_and_group_gaps(seed, first_slots):
    """The ring's flush schedule with rows no fold ever touches and envelopes that do not overlap."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    rng = np.random.default_rng(seed)
    prob = _drop_views(synth.make_problem(40, 500, 15, seed=seed), rng, only_first_slots=first_slots)
    ref = oracle.update(prob, dense_noise=False)
    with UpdateEngine(max_clones=40, max_features=500, max_track=15) as e:
        res = e.update_problem(prob)
        assert res.status == ref["status"] == 0
        assert np.array_equal(res.accepted, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
        T, rn = e.debug_compressed()
        assert not np.triu(T, 90).any()


@pytest.mark.parametrize("seed,first_slots", [(41, None), (42, {0, 1, 9, 10, 17}), (43, {5})])
def test_band_pipeline_tracks_with_holes_and_group_gaps(eng, seed, first_slots):
    """Tracks that skip clones (zero column blocks inside a window) and batches whose tracks start at a few
    slots only (R rows no fold ever touches, folds whose envelopes do not overlap)."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    rng = np.random.default_rng(seed)
    prob = _drop_views(synth.make_problem(28, 400, 10, seed=seed), rng, only_first_slots=first_slots)
    ref = oracle.update(prob, dense_noise=False)
    res = eng.update_problem(prob)
    assert res.status == ref["status"] == 0
    assert np.array_equal(res.accepted, ref["accepted"])
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
    T, rn = eng.debug_compressed()
    assert not np.triu(T, 60).any()                  # band plan taken (every track spans <= 10 slots)


@pytest.mark.parametrize("N,F,M,shards,kw", [
    (30, 2000, 10, 2, {}),
    (30, 2000, 10, 8, {}),
    (20, 500, 8, 3, {"outlier_fraction": 0.1, "outlier_px": 500.0}),
    (12, 60, 10, 4, {"variable_tracks": True}),          # shards without tracks at some first slots
    (30, 700, 10, 16, {}),                               # more records than fold slots: two rounds per group
])
def test_group_exchange_shards_on_one_gpu(N, F, M, shards, kw):
    """Sharded band pipeline: every logical shard exports its group triangles (no root sweep of its own), the
    root folds them group by group, runs ONE root sweep and K6-K7 -- equal to the single-shard update."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import partition_features
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(N, F, M, seed=51, **kw)
    ref = oracle.update(prob, dense_noise=False)
    with UpdateEngine(max_clones=N, max_features=F, max_track=max(M, 2)) as e:
        assert e.band_ok(prob)
        e.set_group_exchange(True)
        recs, total, acc = [], 0, np.zeros(prob.F, dtype=np.uint8)
        for lo, hi in partition_features(prob.view_ptr, shards):
            e.load(prob.subset(lo, hi))
            e.run_compress()
            rec, n = e.export_groups()
            acc[lo:hi] = e.result().accepted
            recs.append(rec); total += n
        e.set_state(prob)
        for it in range(2):                                  # the second call reuses the cached merge plan
            e.merge_groups(np.stack(recs), total if it == 0 else -1)   # -1: the counts the shards wrote into the records
            res = e.result()
            assert res.status == 0 and np.array_equal(acc, ref["accepted"])
            assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
        # a full single-rank update still works on an engine in exchange mode (its own root sweep runs)
        one = e.update_problem(prob)
        assert rel_err(one.dx, ref["dx"]) < TOL and rel_err(one.P_new, ref["P_new"]) < TOL


def _shipped_merge(e, prob, shards, ref, tol_dx=TOL, tol_P=TOL):
    """The exact call sequence of `RcclShardedUpdate.load / step / result` with S logical shards on ONE engine: every
    shard's record is copied (in HBM) into slot r of the exchange buffer -- what the RCCL gather does --, rank 0's
    `merge_groups_flags` with the flags of the partition, then the shared result range is read the way every rank
    reads it after the broadcast."""
    from msckf_amd.shard import shard_group_flags
    bounds = np.array([sh[0] for sh in shards] + [shards[-1][1]], dtype=np.int32)
    e.set_group_exchange(True)
    e.set_exchange_span(e.max_span(prob))                     # every shard: the record layout of the whole batch's sweep mode
    e.set_exchange_mask(bounds)
    count = None
    recv = 0
    for r, (lo, hi) in enumerate(shards):
        e.load(prob.subset(lo, hi))
        if count is None:
            count = e.group_record_doubles()
            recv = e.comm_buffer(count * (len(shards) + 1) + 8)
        assert e.group_record_doubles() == count
        e.run_compress()
        assert e.device_pointer(3) != 0                       # the record heads the workspace, also for a shard without tracks
        e.export_groups(dst_ptr=recv + 8 * count * r, count=False)
    e.set_state(prob)
    flags = shard_group_flags(prob, shards)
    for it in range(2):                                       # the second call reuses the cached merge plan
        e.merge_groups_flags(recv, len(shards), flags)
        assert e.result_range_doubles() == 8 + prob.d + prob.d ** 2 + (prob.F + 7) // 8
        res = e.shared_result()
        assert res.status == ref["status"]
        assert np.array_equal(res.accepted, ref["accepted"])
        assert res.stats["n_accepted"] == int(ref["accepted"].sum())
        assert res.n_rejected == prob.F - int(ref["accepted"].sum())
        if ref["status"] == 0:
            assert rel_err(res.dx, ref["dx"]) < tol_dx and rel_err(res.P_new, ref["P_new"]) < tol_P
        else:
            assert not res.dx.any() and np.array_equal(res.P_new, prob.P)
    e.set_exchange_mask(None)
    e.set_exchange_span(0)
    e.set_group_exchange(False)
    return res


@pytest.mark.parametrize("N,F,M,S,kw", [
    (30, 2000, 10, 2, {"outlier_fraction": 0.1, "outlier_px": 400.0}),
    (30, 2000, 10, 8, {"outlier_fraction": 0.1, "outlier_px": 400.0}),
    (12, 60, 10, 4, {"variable_tracks": True}),              # shards without tracks at some first slots
    (10, 3, 5, 4, {}),                                       # fewer features than ranks: an empty shard takes part
    (8, 20, 5, 3, {"sigma": 0.01, "pixel_noise": 80.0}),     # nothing passes the gate anywhere: no-op on every rank
    (40, 1200, 10, 4, {}),                                   # N > 37: band R in a ring (k_wsweep<4>), 60-column slots
    (24, 600, 15, 3, {"variable_tracks": True}),             # tracks of up to 15 slots: 90-column slots (k_wsweep<6>), ragged:
                                                             # shards whose own tracks are short lay their records out alike
    (50, 900, 15, 8, {"outlier_fraction": 0.05, "outlier_px": 500.0}),   # N = 50, track 15: ring + 90 columns + two-block K6
])
def test_shipped_merge_path_logical_shards(N, F, M, S, kw):
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import partition_features
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(N, F, M, seed=61, **kw)
    ref = oracle.update(prob, dense_noise=False)
    shards = partition_features(prob.view_ptr, S)
    biggest = max(hi - lo for lo, hi in shards)
    # capacity above N on purpose (the result range follows the CURRENT window) and sized for ONE shard, as a rank's engine
    # is: the gate bytes of the whole batch then do not fit the result range the context was created with -- it grows
    with UpdateEngine(max_clones=N + 3, max_features=max(biggest, 8), max_track=max(M, 2)) as e:
        assert e.band_ok(prob)
        _shipped_merge(e, prob, shards, ref)
        one = e.update_problem(prob.subset(*shards[0]))      # the engine still serves plain updates afterwards
        assert one.status in (0, 1)


def test_merge_nodes_that_share_a_table_and_one_that_does_not(monkeypatch):
    """Rank 0's merge plan takes its root and its merge nodes' tables from the planner's memo (`sweep_root`): cross-rank
    merge nodes with the same folds share one table of the uploaded image.  N = 12, 120 tracks of 2 to 6 views over three
    shards cut so that the groups of slots 0, 1, 2 (windows of ten slots: equal triangles) get a triangle from every shard and
    others from two: equal to the oracle, and bit for bit the merge of an engine that keeps no memo."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import shard_group_flags
    from oracle import msckf_oracle as oracle
    N = 12
    prob = synth.make_problem(N, 120, 6, seed=71, variable_tracks=True)
    ref = oracle.update(prob, dense_noise=False)
    shards = [(0, 30), (30, 50), (50, 120)]
    per_group = shard_group_flags(prob, shards).sum(axis=0)
    assert (per_group[:N - 10 + 1] == 3).sum() >= 2 and (per_group == 2).sum() >= 1 and (per_group[:N - 10 + 1] == 2).sum() == 0
    results = []
    for memo in (True, False):
        if not memo:
            monkeypatch.setenv("MSCKF_PLAN_MEMO", "0")
        with UpdateEngine(max_clones=N, max_features=128, max_track=6) as e:
            assert e.band_ok(prob)
            results.append(_shipped_merge(e, prob, shards, ref))
    a, b = results
    assert a.status == b.status == 0
    assert np.array_equal(a.dx, b.dx) and np.array_equal(a.P_new, b.P_new) and np.array_equal(a.accepted, b.accepted)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_shipped_merge_path_config5_full_size(dtype):
    """BASELINE.json configs[4] (N = 50, 20000 features, track 15) split over 8 logical shards, in fp64 and as specified
    (fp32 storage + f32 MFMA P-update): group records with 90-column slots, rank 0 folds them with k_wsweep<6> and runs
    ONE ring-buffered root sweep and the two-block K6 -- no root blocks through host memory, no k_fold_g levels."""
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import partition_features
    prob, ref = _big_case(50, 20000, 15)
    tol = (TOL, TOL) if dtype == "f64" else (1e-4, 1e-5)      # tolerance of the fp32 mode: tests/test_gpu_f32.py
    with UpdateEngine(max_clones=50, max_features=20000, max_track=15, dtype=dtype) as e:
        assert e.band_ok(prob)
        _shipped_merge(e, prob, partition_features(prob.view_ptr, 8), ref, *tol)


@pytest.mark.parametrize("S", [2, 4, 8])
def test_shipped_merge_path_config4_full_size(S):
    """BASELINE.json configs[3] (30, 8000, 10) through the calls `RcclShardedUpdate.step()` makes on rank 0."""
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import partition_features
    prob, ref = _big_case(30, 8000, 10)
    with UpdateEngine(max_clones=30, max_features=8000, max_track=10) as e:
        _shipped_merge(e, prob, partition_features(prob.view_ptr, S), ref)


def test_result_range_follows_the_current_window():
    """`dx | P_out` is ONE contiguous range for the CURRENT N, also when the engine was created for more clones
    (round-2 advisor finding: the range was seated for max_clones, a broadcast of d + d*d doubles then carried a gap
    and a truncated P+)."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    prob = synth.make_problem(12, 200, 6, seed=62)
    with UpdateEngine(max_clones=30, max_features=256, max_track=8) as e:
        e.load(prob)
        e.run()
        res = e.result()
        d = prob.d
        assert e.device_pointer(1) - e.device_pointer(0) == 8 * d
        flat = e.comm_get(e.device_pointer(0), d + d * d)
        assert np.array_equal(flat[:d], res.dx) and np.array_equal(flat[d:].reshape(d, d), res.P_new)
        dx2, P2 = e.result_host()
        assert np.array_equal(dx2, res.dx) and np.array_equal(P2, res.P_new)
        # the window grows: the range is re-seated
        big = synth.make_problem(20, 200, 6, seed=63)
        e.load(big)
        e.run()
        r2 = e.result()
        assert e.device_pointer(1) - e.device_pointer(0) == 8 * big.d
        dx3, P3 = e.result_host()
        assert np.array_equal(dx3, r2.dx) and np.array_equal(P3, r2.P_new)


def test_group_exchange_refuses_tree_planned_batches(eng):
    from msckf_amd import synth
    from msckf_amd._ffi import EngineError
    prob = synth.make_problem(16, 120, 16, seed=36)          # tracks of 16 slots: wider than the sweep tiles, merge tree
    assert not eng.band_ok(prob)
    eng.set_group_exchange(True)
    try:
        eng.load(prob)
        eng.run_compress()
        with pytest.raises(EngineError):
            eng.export_groups()
        blk, n = eng.export_block()                          # the block exchange still works
        assert blk.shape == (96, 97) and n > 0
    finally:
        eng.set_group_exchange(False)



# ---- regressions for the round-1 review ------------------------------------------------------

def test_failed_upload_invalidates_the_previous_batch(eng):
    """A batch that fails validation must not leave the previous batch standing: run() after the failed
    upload returns MSCKF_ERR_STATE instead of launching over buffers sized for another F."""
    from msckf_amd import synth
    from msckf_amd._ffi import EngineError, ERR_DUP_SLOT, ERR_STATE, ERR_ARG
    good = synth.make_problem(12, 40, 6, seed=61)
    eng.load(good)
    eng.run()
    assert eng.result().status == 0
    bad = synth.make_problem(12, 400, 6, seed=62)            # larger than the good batch
    slots = bad.obs_slot.copy()
    a = int(bad.view_ptr[350])
    slots[a + 1] = slots[a]                                  # a track observes the same clone twice
    bad.obs_slot = slots
    with pytest.raises(EngineError) as ei:
        eng.set_features(bad)
    assert ei.value.code == ERR_DUP_SLOT
    with pytest.raises(EngineError) as ei:
        eng.run()
    assert ei.value.code == ERR_STATE
    with pytest.raises(EngineError) as ei:
        eng.run_compress()
    assert ei.value.code == ERR_STATE
    bad2 = synth.make_problem(12, 50, 6, seed=63)
    vp = bad2.view_ptr.copy(); vp[0] = 1                      # CSR must start at 0
    bad2.view_ptr = vp
    with pytest.raises(EngineError) as ei:
        eng.set_features(bad2)
    assert ei.value.code == ERR_ARG
    with pytest.raises(EngineError):
        eng.run()
    eng.set_features(good)                                   # and the engine recovers
    eng.run()
    assert eng.result().status == 0


def test_commit_refuses_a_failed_cholesky(eng):
    """S not positive definite: get_result reports MSCKF_ERR_NOT_SPD and hands back the prior;
    commit_covariance must do the same instead of copying the garbage P_out over the resident prior."""
    from msckf_amd import synth
    from msckf_amd._ffi import EngineError, ERR_NOT_SPD
    prob = synth.make_problem(30, 300, 10, seed=64)
    # indefinite P whose 10-clone diagonal blocks stay SPD: a huge coupling between clone 0 and clone 29
    # (no track sees both, so every per-feature gate passes; the 180 x 180 innovation covariance is indefinite)
    P = 1e-3 * np.eye(prob.d)
    P[15, 15 + 6 * 29] = P[15 + 6 * 29, 15] = 50.0
    P[18, 18 + 6 * 29] = P[18 + 6 * 29, 18] = -50.0
    prob.P = P
    eng.load(prob)
    eng.run()
    with pytest.raises(EngineError) as ei:
        eng.result()
    assert ei.value.code == ERR_NOT_SPD
    with pytest.raises(EngineError) as ei:
        eng.commit_covariance()
    assert ei.value.code == ERR_NOT_SPD
    assert np.array_equal(eng.covariance(), P)               # the resident prior is untouched


def test_band_rule_comes_from_the_library():
    """The exchange format of a sharded update is the library's own rule (msckf_band_rule): it follows the
    engine's plan flag and tile limits, so a tree-planned engine never promises group records."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import HipShardBackend
    narrow = synth.make_problem(30, 200, 10, seed=1)
    with UpdateEngine(max_clones=64, max_features=500, max_track=31) as e:
        assert e.band_ok(narrow)
        assert e.band_ok(synth.make_problem(12, 40, 10, seed=2, variable_tracks=True))
        assert e.band_ok(synth.make_problem(45, 300, 10, seed=4))              # N > 37: band R in a ring
        assert e.band_ok(synth.make_problem(20, 100, 15, seed=5))              # tracks of 15 slots: 90-column tiles
        assert not e.band_ok(synth.make_problem(20, 60, 16, seed=6))           # 16 slots: wider than the tiles
        assert not e.band_ok(synth.make_problem(40, 40, 31, seed=3))           # tracks of 31 slots: merge tree
        assert not e.band_ok(synth.make_problem(5, 0, 3, seed=0))              # empty batch
    with UpdateEngine(max_clones=30, max_features=500, max_track=10, plan="tree") as e:
        assert not e.band_ok(narrow)
        be = HipShardBackend(e)
        be.prepare(narrow)
        assert not be.groups
        blk, n, acc = be.compress(narrow)                                       # block exchange on a tree-planned engine
        assert blk.shape == (180, 181) and n == int(acc.sum()) > 0


# ---- BASELINE.json configs[3] and configs[4] at full size ------------------------------------------

_BIG = {}


def _big_case(N, F, M):
    """Problem + oracle result, computed once per session (the oracle takes tens of seconds at these sizes)."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    key = (N, F, M)
    if key not in _BIG:
        prob = synth.make_problem(N, F, M, seed=0)
        _BIG[key] = (prob, oracle.update(prob, dense_noise=False))
    return _BIG[key]


@pytest.mark.parametrize("shards", [2, 4, 8])
def test_config4_full_size_sharded(shards):
    """BASELINE.json configs[3]: N = 30, 8000 features, track 10, feature-sharded 2 / 4 / 8 ways.  Logical shards
    on one GPU: every shard exports its records, the root merges them (two-level group merges at this size),
    runs one root sweep and K6-K7; against the oracle on the whole batch."""
    from msckf_amd.api import UpdateEngine
    from msckf_amd.shard import partition_features
    prob, ref = _big_case(30, 8000, 10)
    with UpdateEngine(max_clones=30, max_features=8000, max_track=10) as e:
        groups = e.band_ok(prob)
        e.set_group_exchange(groups)
        recs, total, acc = [], 0, np.zeros(prob.F, dtype=np.uint8)
        for lo, hi in partition_features(prob.view_ptr, shards):
            e.load(prob.subset(lo, hi))
            e.run_compress()
            rec, n = e.export_groups() if groups else e.export_block()
            acc[lo:hi] = e.result().accepted
            recs.append(rec); total += n
        e.set_state(prob)
        if groups:
            e.merge_groups(np.stack(recs), -1)
        else:
            e.merge_gain(np.stack(recs), total)
        res = e.result()
        assert res.status == 0 and total == int(ref["accepted"].sum())
        assert np.array_equal(acc, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
        e.set_group_exchange(False)
        one = e.update_problem(prob)                         # and the unsharded update of the same batch
        assert rel_err(one.dx, ref["dx"]) < TOL and rel_err(one.P_new, ref["P_new"]) < TOL


def test_config5_full_size_fp64():
    """BASELINE.json configs[4] in fp64: N = 50, 20000 features, track 15 (d = 315, 540000 stacked rows)."""
    from msckf_amd.api import UpdateEngine
    prob, ref = _big_case(50, 20000, 15)
    with UpdateEngine(max_clones=50, max_features=20000, max_track=15) as e:
        res = e.update_problem(prob)
        assert res.status == 0
        assert np.array_equal(res.accepted, ref["accepted"])
        assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
        assert np.array_equal(res.P_new, res.P_new.T)


@pytest.mark.parametrize("M", list(range(2, 32)))
def test_gate_statistic_of_long_tracks(M):
    """gamma of every track against the oracle at 1e-9 for EVERY track length the engine takes (2 - 31 views: the three
    instances of k_feature and all their column-chunk boundaries; reference MSCKF.py:561-568).  Tracks of exactly 21 and 31 views were split into chunks of 11 views = 66 columns on 64
    lanes until round 4: the gate lost two columns of one view, gamma was off by a few per cent -- and by a factor of 50 for a
    track whose gross outlier sat in that view, which the gate then accepted."""
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    N = max(M, 25)
    prob = synth.make_problem(N, 160, M, seed=900 + M, outlier_fraction=0.3, outlier_px=300.0, min_track=2)
    ref = oracle.update(prob, dense_noise=False)
    with UpdateEngine(max_clones=31, max_features=256, max_track=31) as eng:
        res = eng.update_problem(prob)
        gam, _ = eng.debug_gate()
    np.testing.assert_allclose(gam, ref["gamma"], rtol=1e-9, atol=1e-12)
    assert 0 < int(ref["accepted"].sum()) < prob.F                       # both sides of the gate are populated
    assert np.array_equal(res.accepted, ref["accepted"])
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL


@pytest.mark.parametrize("N", list(range(1, 54)))
def test_every_window_size(eng, N):
    """One small batch per window size 1 - 53 against the oracle: strip counts 2 - 21 of the streamed K6-K7, every length of its
    short first row block (6 N mod 16), the sweep forms on either side of N = 37 and the wide-track rule on either side of N = 31.
    Windows of 54 clones and more: tests/test_gpu_wide_windows.py."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    M = max(1, min(N, 2 + N % 9))
    prob = synth.make_problem(N, 90, M, seed=1300 + N, variable_tracks=M > 2, outlier_fraction=0.15, outlier_px=300.0)
    ref = oracle.update(prob, dense_noise=False)
    res = eng.update_problem(prob)
    assert res.status == ref["status"] and np.array_equal(res.accepted, ref["accepted"])
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL
    if res.status == 0:
        assert np.array_equal(res.P_new, res.P_new.T)


@pytest.mark.parametrize("F", [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 239, 240, 241, 255, 256, 257, 383, 511, 513])
def test_batch_sizes_around_the_plan_boundaries(eng, F):
    """Batch sizes on either side of the leaf / row-block / wavefront counts of the K5 plan (features per row block, blocks per
    round, leaves per group, the streamed merge level appearing and disappearing) against the oracle."""
    from msckf_amd import synth
    from oracle import msckf_oracle as oracle
    prob = synth.make_problem(30, F, 10, seed=2100 + F, variable_tracks=(F % 2 == 1), outlier_fraction=0.1 if F > 8 else 0.0, outlier_px=300.0)
    ref = oracle.update(prob, dense_noise=False)
    res = eng.update_problem(prob)
    assert res.status == ref["status"] and np.array_equal(res.accepted, ref["accepted"])
    assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL


@pytest.mark.parametrize("case", ["few_rows_wide_tracks_283", "few_rows_wide_tracks_373"])
def test_wide_tracks_with_few_rows_fall_back_to_householder(case):
    """Two synthetic batches found by tools/soak_holes.py (tests/regress/*.npz hold their inputs): short tracks with holes that span
    more than 10 clone slots but contribute far fewer rows than the window has columns.  Round 4's information form met a
    non-positive pivot on them (rank of the Gram matrix << 6N + 1) and had to re-plan; since round 5 such tracks are split
     and every row is a Householder row.  Kept: the one-shot call, the resident sequence committing unseen, the
    exported block (one plan for every block) and `plan="band"` (no split) must agree with the oracle and with each other."""
    import os
    from msckf_amd import synth
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    d = np.load(os.path.join(os.path.dirname(__file__), "regress", case + ".npz"))
    prob = synth.UpdateProblem(**{k: d[k] for k in d.files})
    prob.sigma = float(prob.sigma)
    ref = oracle.update(prob, dense_noise=False)
    assert ref["status"] == 0
    with UpdateEngine(max_clones=53, max_features=2048, max_track=31) as eng:
        res = eng.update_problem(prob)
        eng.load(prob)                                       # the resident sequence, committing without looking at the result
        eng.run()
        assert eng.commit_covariance() == 0
        P_committed = eng.covariance()
        eng.load(prob)                                       # the block that leaves the context: one plan for every track
        eng.run_compress()
        T1, r1 = eng.debug_compressed()
    with UpdateEngine(max_clones=53, max_features=2048, max_track=31, plan="band") as eng:
        band = eng.update_problem(prob)
        T0, r0 = eng.debug_compressed()
    for r in (res, band):
        assert r.status == 0 and np.array_equal(r.accepted, ref["accepted"])
        assert rel_err(r.dx, ref["dx"]) < TOL and rel_err(r.P_new, ref["P_new"]) < TOL
    assert rel_err(P_committed, ref["P_new"]) < TOL
    # (the merge tree over a batch that is sorted class by class: its leaves must not straddle a class boundary -- until round 4
    #  they did, and msckf_run_compress handed out a wrong block for such a batch)
    assert rel_err(T1.T @ T1, T0.T @ T0) < 1e-10 and rel_err(T1.T @ r1, T0.T @ r0) < 1e-10


def test_ragged_tracks_soak():
    """tools/soak_holes.py's generator, 60 batches: every track a random subset of the views of a full-window track (holes, any
    span, 2 - 31 views), window sizes 2 - 53, up to 40 % outliers -- the shapes of `MSCKF.py:404-412`'s track bookkeeping rather than
    the benchmark's consecutive views.  One-shot call against the oracle."""
    import importlib.util, os
    from msckf_amd.api import UpdateEngine
    from oracle import msckf_oracle as oracle
    spec = importlib.util.spec_from_file_location("soak_holes", os.path.join(os.path.dirname(__file__), "..", "tools", "soak_holes.py"))
    sh = importlib.util.module_from_spec(spec); spec.loader.exec_module(sh)
    rng = np.random.default_rng(11)
    with UpdateEngine(max_clones=53, max_features=2048, max_track=31) as eng:
        for c in range(60):
            N = int(rng.integers(2, 54)); F = int(rng.integers(1, 200))
            hi = int(rng.integers(2, min(N, 31) + 1))
            prob = sh.ragged(rng, N, F, 2, hi, float(rng.choice([0.0, 0.1, 0.4])))
            ref = oracle.update(prob, dense_noise=False)
            res = eng.update_problem(prob)
            gam, _ = eng.debug_gate()
            assert res.status == ref["status"] and np.array_equal(res.accepted, ref["accepted"]), (c, N, F, hi)
            np.testing.assert_allclose(gam, ref["gamma"], rtol=1e-7, atol=1e-11, err_msg=str((c, N, F, hi)))
            if res.status == 0:
                assert rel_err(res.dx, ref["dx"]) < TOL and rel_err(res.P_new, ref["P_new"]) < TOL, (c, N, F, hi)
