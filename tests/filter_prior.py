"""Filter-shaped priors for the update and the resident kernels, the metrics that read them in covariance units, and the one
table of GPU cases that runs on them.  Host only, NumPy; not a conftest: imported by name.

Recipe A (`synth.random_spd_covariance`) gives every state the same sigma and almost no correlation.  A covariance that a filter
produced is different: the newest clone is an exact function of the IMU state (singular, correlations of 1.0), sigma spans
gyro bias to position.  The suite held such a prior only as fixtures of 10 - 30 clones (`*_B`); `filter_prior` builds one of any
width from the project's own host functions and the `seq_short` fixture's head (P0, Qc and the extrinsics: the reference's scales).

  filter_prior(N, seed)   (P, cam_R, cam_t, ops, imu) after N frames along `synth.clone_poses`' trajectory
  scaled_P, scaled_dx,    entrywise errors over the sigmas of the entry, and `rel_err` on the update term P - P+: what a
  update_term             Frobenius norm over the whole array cannot see on such a prior (tests/test_filter_prior.py, section 3)
  CASES                   name -> Case; tests/test_filter_prior.py holds every entry to its conditions on the CPU,
                          tests/test_gpu_filter_prior.py runs them on the engine
"""
import functools
from collections import namedtuple

import numpy as np

from conftest import load_sequence, rel_err
import nominal_ref

MAX_N = 221
# The clock.  Frames are 0.1 s apart (a 10 Hz camera) while the window spans at most 3 s; a wider window covers the same 3 s
# with more frames.  At 0.1 s max sigma / min sigma comes out at 103 / 209 / 454 for 10 / 20 / 30 clones with position at
# 0.45 m, and the reference's own priors (cfg1_B, cfg2_B, edge_long_tracks_B: 10 / 20 / 30 clones) have 102 / 205 / 446:
# tests/test_filter_prior.py pins the two to each other.  Both ends of the choice were measured on the CPU, on the reference
# spread alone (two exact fp64 algorithms against each other, `spread` below): at the 30 ms of seq_short a short-track update
# on 10 clones removes 2e-4 of |P|, which leaves the update-term measure a floor of eps / 2e-4 = 2e-12 in ANY fp64 arithmetic;
# 0.1 s carried on to 221 frames is a filter that dead-reckoned for 22 s (position sigma 30 m, sigma ratio 3e4), where the two
# algorithms differ by up to 2e-9 on dx.  No filter holds either state; 3 s is the span of the widest prior the reference made.
FRAME_DT, SPAN = 0.1, 3.0
PRIOR_SEED = 1
KEPT = (1, 2, 3, 10, 11, 53, 54, 82, 83, 128, 220, 221)       # the widths at which a run keeps its covariance on the way


def frame_dt(N):
    return min(FRAME_DT, SPAN / max(N, 1))


# ---- the generator ------------------------------------------------------------------------------------------------------------

class _Run:
    """One seeded run of N frames: frame i is `steps` IMU samples (`propagation.imu_transition` ->
    `oracle.propagate_covariance`) and one `propagation.augmentation` -> `oracle.augment_covariance`."""

    def __init__(self, N, seed, steps, frame):
        from msckf_amd import propagation, synth
        from oracle import msckf_oracle as oracle
        head, _ = load_sequence("seq_short")
        self.head = head
        cam_R, cam_t = synth.clone_poses(N, np.random.default_rng([seed, 0]))
        T_W_I, T_W_C = (head["T_W_I_R"], head["T_W_I_t"]), (head["T_W_C_R"], head["T_W_C_t"])
        R_IC, t_IC = propagation.extrinsics(T_W_I, T_W_C)
        # the IMU pose of a frame: the clone pose taken back through the extrinsics, T_W_I = T_W_C T_I_C^-1
        imu_R = [R @ R_IC.T for R in cam_R]
        imu_t = [t - Ri @ t_IC for t, Ri in zip(cam_t, imu_R)]
        g = np.asarray(head["gravity"], dtype=np.float64)
        rng = np.random.default_rng([seed, 1])
        dt = frame / steps
        P = np.array(head["P0"], dtype=np.float64)
        self.ops, self.samples, self.kept = [], [], {}
        for i in range(N):
            # the IMU starts from the pose of the frame before (the first frame: its own) with the velocity that carries it to
            # this frame's position; the clone is taken at this frame's pose
            j = max(i - 1, 0)
            R, t = imu_R[j], imu_t[j]
            v = (imu_t[i] - t) / frame + 0.01 * rng.standard_normal(3)
            for _ in range(steps):
                gyro = 0.05 * rng.standard_normal(3)                           # small random rates
                acc = R.T @ (g + 0.05 * rng.standard_normal(3))                # the specific force of a nearly unaccelerated body,
                R0, t0, v0 = R, t, v                                           # in IMU.integrate's convention a = R acc - g
                R, t, v, _ = nominal_ref.integrate(R, t, v, acc, gyro, dt, g, np.zeros(3))
                Phi, Q = propagation.imu_transition(R, t, v, R0, t0, v0, gyro, acc, dt, g, head["Qc"])
                P = oracle.propagate_covariance(P, Phi, Q)
                self.ops.append(("propagate", Phi, Q))
                self.samples.append(dict(gyro=gyro, acc=acc, dt=dt, R=R, t=t, v=v, R0=R0, t0=t0, v0=v0))
            J, cR, ct = propagation.augmentation(imu_R[i], imu_t[i], T_W_I, T_W_C)
            P = oracle.augment_covariance(P, J)
            self.ops.append(("augment", J, cR, ct))
            if i + 1 in KEPT or i + 1 == N:
                P.setflags(write=False)
                self.kept[i + 1] = P
        self.P = P
        self.cam_R = np.array([op[2] for op in self.ops if op[0] == "augment"]).reshape(N, 3, 3)
        self.cam_t = np.array([op[3] for op in self.ops if op[0] == "augment"]).reshape(N, 3)


@functools.lru_cache(maxsize=None)
def _run(N, seed, steps, frame):
    return _Run(N, seed, steps, frame)


def filter_prior(N, seed=PRIOR_SEED, steps=2, frame=None):
    """(P, cam_R, cam_t, ops, imu) of a filter that ran N frames (0 <= N <= 221), `frame` seconds apart (default: frame_dt(N),
    the clock above).  Memoised per argument tuple.

    P        (15 + 6 N)^2, read-only (copy before changing it)
    cam_R/t  the N clone poses, as `propagation.augmentation` returned them (synth.clone_poses' up to one rounding)
    ops      the N (steps + 1) operations that built P from the fixture's P0, in order: ("propagate", Phi, Q) and
             ("augment", J, cam_R, cam_t) -- what `eng.propagate` / `eng.augment` take
    imu      per IMU sample a dict of the raw sample (gyro, acc, dt; the biases are zero), the state after it (R, t, v) and
             the null state before it (R0, t0, v0); imu[k] belongs to the k-th "propagate" of ops"""
    if not 0 <= N <= MAX_N:
        raise ValueError(f"N = {N} outside 0 .. {MAX_N}")
    run = _run(N, seed, steps, frame_dt(N) if frame is None else float(frame))
    return run.P, run.cam_R, run.cam_t, run.ops, run.samples


def on_the_way(N, n, seed=PRIOR_SEED, steps=2):
    """The covariance of filter_prior(N)'s run when it held n clones (n in KEPT or n = N)."""
    return _run(N, seed, steps, frame_dt(N)).kept[n]


def head():
    """The `seq_short` fixture's head: P0, Qc, gravity, K, sigma, T_W_I_*, T_W_C_*."""
    return _run(0, PRIOR_SEED, 2, FRAME_DT).head


def replay(ops, P0):
    """`ops` through the oracle's covariance steps."""
    from oracle import msckf_oracle as oracle
    P = np.array(P0, dtype=np.float64)
    for op in ops:
        P = oracle.propagate_covariance(P, op[1], op[2]) if op[0] == "propagate" else oracle.augment_covariance(P, op[1])
    return P


def statistics(P):
    """(smallest, largest eigenvalue of the correlation matrix, largest off-diagonal correlation, max sigma / min sigma)."""
    s = np.sqrt(np.diag(P))
    C = P / np.outer(s, s)
    ev = np.linalg.eigvalsh((C + C.T) / 2)
    off = np.abs(C - np.diag(np.diag(C))).max() if P.shape[0] > 1 else 0.0
    return float(ev[0]), float(ev[-1]), float(off), float(s.max() / s.min())


# ---- the metrics --------------------------------------------------------------------------------------------------------------

def scaled_P(got, ref):
    """max |got - ref|_ij / sqrt(ref_ii ref_jj): the error of every entry in units of the two sigmas it belongs to."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    s = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(got - ref) / np.outer(s, s)))


def scaled_dx(got, ref, P_prior):
    """max |got - ref|_i / sqrt(P_prior_ii): the error of every correction in units of the prior sigma of its state."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.sqrt(np.diag(P_prior))))


def update_term(got, ref, P_prior):
    """`rel_err` on what the update subtracted, P - P+: the part of P+ the kernels computed, without the prior beside it."""
    P = np.asarray(P_prior, dtype=np.float64)
    return rel_err(P - np.asarray(got, dtype=np.float64), P - np.asarray(ref, dtype=np.float64))


def metrics(dx, P_new, ref, P_prior):
    """(e_dx, e_P, s_dx, s_P, u_P) of an update against the oracle's `ref`."""
    return (rel_err(dx, ref["dx"]), rel_err(P_new, ref["P_new"]), scaled_dx(dx, ref["dx"], P_prior),
            scaled_P(P_new, ref["P_new"]), update_term(P_new, ref["P_new"], P_prior))


# ---- the cases ----------------------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "name family N F M kind base key")

# kind -> the batch on the prior.  short / full / long: tests/test_gpu_wide_windows.py's helpers; plan:
# test_batch_sizes_around_the_plan_boundaries' batch; few: test_chain_fewest_features_at_capacity's.
SEED_BASE = {"forms": 20000, "stream": 20300, "chain": 20600, "few": 20900, "long": 21200, "plan": 21500, "forced": 21800,
             "device": 22100, "inject": 22400}
# Seeds follow tests/test_f32_model.py's rule: base + key + 1000 k with the first k at which the case meets every condition of
# tests/test_filter_prior.py (status 0, both sides of the gate populated, no verdict within 1e-6 of the threshold, reference
# spread <= 1e-12 in all four measures).  Every case whose k is not 0, with what k = 0 .. missed:
SEED_SKIPS = {}


def _cases():
    out = []
    add = lambda family, name, N, F, M, kind, key: out.append(Case(name, family, N, F, M, kind, SEED_BASE[family], key))
    for N in (1, 2, 10, 11, 21, 22, 31, 32, 37, 38, 53):       # the solve dispatch of K6-K7 below 54 clones, the band ring past 37
        add("forms", f"forms_{N}", N, 90, max(1, min(N, 2 + N % 9)), "short", N)
    for N in (54, 64, 65, 82):                                 # the streamed K6-K7
        add("stream", f"stream_{N}", N, 4 * N, max(1, min(N, 2 + N % 9)), "short", N)
    for N in (83, 107, 187, 221):                              # the chain, T full
        add("chain", f"chain_{N}", N, max(90, 2 * N), 10, "full", N)
    for F in (1, 2):
        add("few", f"chain_221_F{F}", MAX_N, F, 8, "few", F)
    for N in (31, 53, 64, 65, 107):                            # tracks of 11 - 31 views: split up to N = 64, the merge tree past it
        add("long", f"long_{N}", N, 60, 31, "long", N)
    for F in (1, 16, 17, 64, 65, 256, 257):                    # the K5 plan's boundaries
        add("plan", f"plan_{F}", 30, F, 10, "plan", F)
    for N in (10, 11, 21, 22, 31, 32, 53, 54, 82):             # MSCKF_GAIN_STREAM=0: the chain where the default never takes it
        add("forced", f"forced_{N}", N, max(90, 2 * N), 10, "full", N)
    add("device", "device_221", MAX_N, 2 * MAX_N, 10, "full", MAX_N)   # on the prior the device built (the oracle's, on the CPU)
    for N in (64, 65, 221):                                    # the update before the injection past lane 64
        add("inject", f"inject_{N}", N, 90, max(1, min(N, 2 + N % 9)), "short", N)
    return {c.name: c for c in out}


CASES = _cases()
NO_ROWS = ("forms_1",)             # a window of one clone: one view per track, no rows -- status 1, the no-op contract
ONE_SIDED = ("chain_221_F1", "chain_221_F2", "plan_1")      # F = 1, 2: a gate with one side only is allowed


def case_seed(case, k=None):
    return case.base + case.key + 1000 * (SEED_SKIPS.get(case.name, (0,))[0] if k is None else k)


def make_case(case, k=None):
    from msckf_amd import synth
    import test_gpu_wide_windows as ww
    seed = case_seed(case, k)
    P, cam_R, cam_t, _, _ = filter_prior(case.N)
    state = dict(P=np.array(P), poses=(cam_R, cam_t))
    if case.kind == "short":
        return ww.short_problem(case.N, seed, F=case.F, **state)
    if case.kind == "full":
        return ww.full_problem(case.N, seed, **state)
    if case.kind == "long":
        return ww.long_problem(case.N, seed, F=case.F, M=case.M, min_track=11, **state)
    if case.kind == "few":
        return synth.make_problem(case.N, case.F, case.M, seed=seed, **state)
    F = case.F
    return synth.make_problem(case.N, F, case.M, seed=seed, variable_tracks=(F % 2 == 1), outlier_fraction=0.1 if F > 8 else 0.0,
                              outlier_px=300.0, **state)


@functools.lru_cache(maxsize=None)
def problem(name, k=None):
    """(prob, oracle result) of a case, computed once and shared: leave both unchanged."""
    from oracle import msckf_oracle as oracle
    prob = make_case(CASES[name], k)
    return prob, oracle.update(prob, dense_noise=False)


def gate_margin(ref):
    """The smallest |gamma - chi2| / chi2 over the features."""
    return float(np.min(np.abs(ref["gamma"] - ref["crit"]) / ref["crit"]))


def spread(prob, ref, samples=4):
    """The reference spread: the engine's sequential 16-row block form in exact fp64 (`f32_model.update` without rounding) on
    the oracle's blocks in a random null-space basis each and in permuted order, against the oracle's MSCKF.py:594-614 form.
    The largest over `samples` draws seeded [0, s] of (scaled_dx, scaled_P, update_term, rel_err on dx)."""
    import f32_model as fm
    blks = fm.blocks(prob, ref)
    worst = np.zeros(4)
    for s in range(samples):
        rng = np.random.default_rng([0, s])
        order = rng.permutation(len(blks))
        dx, Pn = fm.update(fm.stack(prob, ref, rng, [blks[i] for i in order]), prob.P, prob.sigma, False, False)
        e_dx, _, s_dx, s_P, u_P = metrics(dx, Pn, ref, prob.P)
        worst = np.maximum(worst, [s_dx, s_P, u_P, e_dx])
    return tuple(float(x) for x in worst)
