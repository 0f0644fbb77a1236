"""Mixed call sequences on the resident filter: the one table of sequences, built on the CPU by stepping `filter_model.FilterModel`.
Host only, NumPy; not a conftest: imported by name.

A sequence is a list of ops (name, keyword arguments) for `step` (the model) and for the GPU test's `drive` (the engine).  It is
generated deterministically from a seed: every argument that depends on the filter's state -- a camera batch, the rows of a
measurement, a fix -- is drawn on the state the MODEL holds at that point.  Nothing read from a device enters a sequence; the GPU
test rebuilds the same table from the same seeds.

  camera batches   `synth.make_problem(N, F, M, seed, P=<model P>, poses=<model poses>, outlier_fraction=...)`: F <= 40, tracks of
                   2 .. min(M, N) views, 15 % outliers.  A batch is run on the state it was drawn for unless the sequence says
                   otherwise (`batch_lifetime`, the random sequences)
  rows             `rows_ref.rows_on` on the model's P: noise in units of sqrt(diag P), r = chol(S) N(0, I); m from {1, 3, 6, 17};
                   gated ones at gamma (1 +- rows_ref.GATE_REL)
  IMU batches      1 .. 5 raw samples over ~0.1 s, the body of `filter_prior`'s trajectory: small rates, nearly unaccelerated
  sizes            N in 0 .. 8 on contexts of 9 clones (d <= 63: one to four ragged 16-tiles); `refusals_between` on a context of
                   8, which it fills; `long_tracks` at N = 18 .. 20 on a context of 20

NAMED holds the sequences written out by hand, RANDOM the 24 drawn ones.  A random sequence draws 24 ops: with probability
1 / 6 one of the calls that are ILLEGAL in the current state (it must return its error code and change nothing), otherwise one
of the legal ones with the fixed weights of WEIGHTS.  Read-backs (`result`, `covariance`, `nominal`) are ops of the sequence
like any other: they change the engine's path.  `set_state` / `set_nominal` are not drawn (the sequence `reprior` holds them).
A drawn sequence must meet `composition_misses`' rules; its seed is RANDOM_BASE + i + 1000 k with the first k at which it does
and at which tests/test_call_sequences.py's conditions hold (the rule of tests/filter_prior.py); SEED_SKIPS lists every k != 0.
A camera batch is redrawn (`Builder.camera`) until, on the state it is drawn for, some but not all of its features pass the gate
and no verdict is near its critical value; nothing else is redrawn, and no drawn op is ever taken out."""
import dataclasses
import functools
from collections import namedtuple

import numpy as np

import filter_model as fm
import filter_prior as fp
import rows_ref as rr

Sequence = namedtuple("Sequence", "name max_clones ops meta")      # meta[i]: dict(rc, illegal, partial, reject_all) of op i

MAX_CLONES = 9
ROWS_M = (1, 3, 6, 17)
N_RANDOM, RANDOM_OPS, RANDOM_BASE = 24, 24, 26000
ILLEGAL_RATE = 1.0 / 6.0
READBACKS = ("result", "covariance", "nominal")
# the calls that change P, the poses or the nominal record when they return 0
MUTATING = ("set_prior", "set_nominal", "set_poses", "propagate", "propagate_imu", "augment", "augment_imu", "remove_clones",
            "commit_covariance", "commit_inject")
COMMITS = ("commit_covariance", "commit_inject")
UPDATES = ("run", "run_rows", "velocity_fix", "position_fix", "zero_velocity")
WEIGHTS = dict(propagate_imu=1.0, propagate=0.5, augment_imu=5.0, augment=0.3, remove_clones=3.0, set_poses=0.3, set_features=8.0,
               run=30.0, run_rows=7.0, velocity_fix=0.7, position_fix=0.7, zero_velocity=0.7, commit_inject=60.0, commit_covariance=6.0,
               result=14.0, covariance=6.0, nominal=6.0)
# Random sequences whose first seeds missed a rule or a condition: name -> (k, what k = 0, 1, .. missed, one word per seed).  Five rules
# ask a lot of 24 draws, so most first seeds miss one.  a: fewer than three applied updates, r: no rows update, c: no camera update,
# n: no change of N behind an update, b: no commit without a result in front of it (`composition_misses`); w: an update that removes
# less than rows_ref.MIN_UPDATE of |P| (the same measurement drawn again on the P it had just shrunk), s: the two exact forms
# further apart than tests/test_call_sequences.py allows.  tests/test_call_sequences.py recomputes every word.
SEED_SKIPS = {
    "random_00": (8, "a arcnb c w c arcnb n ac"),
    "random_01": (1, "a"),
    "random_02": (21, "ac rn an acn w c arb ar a cn ar arcnb ac n a rn n ac w c ar"),
    "random_03": (9, "ac c acn c a arcnb arcnb ar c"),
    "random_04": (3, "n ac n"),
    "random_05": (5, "c acn c ar arn"),
    "random_06": (2, "ws n"),
    "random_07": (1, "w"),
    "random_08": (4, "a r rn acn"),
    "random_09": (12, "a arcnb w arn n ac w arn w rn acn r"),
    "random_10": (5, "ac r w a rn"),
    "random_11": (4, "c cn n c"),
    "random_13": (4, "n arcnb ar arb"),
    "random_15": (5, "ac n ac ac ac"),
    "random_16": (16, "n rn ac n c n arn w ac acb rn n ac cn arn ac"),
    "random_17": (3, "acn arcnb cn"),
    "random_18": (6, "ac c n sw w arn"),
    "random_19": (2, "c cn"),
    "random_21": (2, "ac n"),
    "random_22": (2, "a arcnb"),
    "random_23": (6, "n c ac arcnb n n"),
}


# ---- one op on the model ---------------------------------------------------------------------------------------------------------

def state_args():
    h = fp.head()
    from msckf_amd import synth
    return dict(gravity=np.asarray(h["gravity"], dtype=np.float64), K=synth.K_DEFAULT.copy(), sigma=0.2)


def extrinsics():
    from msckf_amd import propagation
    h = fp.head()
    return propagation.extrinsics((h["T_W_I_R"], h["T_W_I_t"]), (h["T_W_C_R"], h["T_W_C_t"]))


def step(model, op):
    """One op on a FilterModel: (code, payload); the payload of a read-back is what it read, else None."""
    name, kw = op
    if name == "set_prior":
        return model.set_prior(kw["P"], cam_R=kw["cam_R"], cam_t=kw["cam_t"], cam_R0=kw.get("cam_R0"), cam_t0=kw.get("cam_t0"), **state_args()), None
    if name == "set_nominal":
        h = fp.head()
        return model.set_nominal(kw["R"], kw["t"], kw["v"], state_args()["gravity"], h["Qc"], extrinsics(), b_g=kw.get("b_g"), b_a=kw.get("b_a")), None
    if name in READBACKS:
        return getattr(model, name)()
    if name == "set_features":
        return model.set_features(kw["prob"]), None
    return getattr(model, name)(**kw), None


# ---- the builder -------------------------------------------------------------------------------------------------------------------

class Builder:
    """Steps a model and writes down what it was given."""

    def __init__(self, name, max_clones, N0, seed):
        self.name, self.max_clones = name, max_clones
        self.model = fm.FilterModel(max_clones)
        self.rng = np.random.default_rng([seed, 0])
        self.seed, self.draws = seed, 0
        self.ops, self.meta = [], []
        self.fresh = False                # the loaded batch was drawn on the state the model holds
        self.reprior(N0)

    def op(self, name, expect=None, illegal=False, **kw):
        rc, _ = step(self.model, (name, kw))
        if expect is not None:
            assert rc == expect, (self.name, len(self.ops), name, rc, expect)
        if illegal:
            assert rc < 0, (self.name, len(self.ops), name, rc)
        if name in MUTATING and rc == 0:
            self.fresh = False
        self.ops.append((name, kw))
        self.meta.append(dict(rc=rc, illegal=illegal, partial=False, reject_all=False))
        return rc

    # -- the state
    def reprior(self, N, biases=False):
        P, cam_R, cam_t, _, imu = fp.filter_prior(N)
        self.op("set_prior", expect=0, P=np.array(P), cam_R=np.array(cam_R), cam_t=np.array(cam_t))
        s = fp.filter_prior(max(N, 2))[4][-1]           # (the IMU under way along the trajectory: the first frame starts at rest)
        kw = dict(b_g=1e-3 * self.rng.standard_normal(3), b_a=1e-2 * self.rng.standard_normal(3)) if biases else {}
        self.op("set_nominal", expect=0, R=np.array(s["R"]), t=np.array(s["t"]), v=np.array(s["v"]), **kw)

    def imu(self, n=None, **kw):
        s, g = self.model.nom, state_args()["gravity"]
        n = int(self.rng.integers(1, 6)) if n is None else n
        gyro = 0.05 * self.rng.standard_normal((n, 3)) + s["b_g"]
        acc = (g + 0.05 * self.rng.standard_normal((n, 3))) @ s["R"] + s["b_a"]       # rows R^T (g + noise): nearly unaccelerated
        dt = (0.1 / n) * self.rng.uniform(0.8, 1.2, n)
        return self.op("propagate_imu", gyro=gyro, acc=acc, dt=dt, **kw)

    def host_propagate(self, **kw):
        """Phi, Q of one 20 ms sample from the model's IMU state; the record itself does not move."""
        import nominal_ref
        from msckf_amd import propagation
        s, h, g = self.model.nom, fp.head(), state_args()["gravity"]
        gyro, acc, dt = 0.05 * self.rng.standard_normal(3), s["R"].T @ (g + 0.05 * self.rng.standard_normal(3)), 0.02
        R, t, v, _ = nominal_ref.integrate(s["R"], s["t"], s["v"], acc, gyro, dt, g, np.zeros(3))
        Phi, Q = propagation.imu_transition(R, t, v, s["R"], s["t"], s["v"], gyro, acc, dt, g, h["Qc"])
        return self.op("propagate", Phi=Phi, Q=Q, **kw)

    def host_augment(self, **kw):
        """The clone of an IMU pose 0.1 s ahead of the record's, in the caller's form (J, R, t)."""
        from msckf_amd import propagation
        s, h = self.model.nom, fp.head()
        J, R, t = propagation.augmentation(s["R"], s["t"] + 0.1 * s["v"], (h["T_W_I_R"], h["T_W_I_t"]), (h["T_W_C_R"], h["T_W_C_t"]))
        return self.op("augment", J15=J, R=R, t=t, **kw)

    def poses(self, **kw):
        """Poses a host injection might have left, with null poses of their own."""
        from msckf_amd import synth
        m, N = self.model, self.model.N
        R = np.stack([synth.so3_exp(1e-3 * self.rng.standard_normal(3)) @ m.cam_R[i] for i in range(N)]) if N else np.zeros((0, 3, 3))
        t = m.cam_t + 1e-3 * self.rng.standard_normal((N, 3))
        R0 = np.stack([synth.so3_exp(5e-3 * self.rng.standard_normal(3)) @ R[i] for i in range(N)]) if N else np.zeros((0, 3, 3))
        t0 = t + 1e-2 * self.rng.standard_normal((N, 3))
        return self.op("set_poses", cam_R=R, cam_t=t, cam_R0=R0, cam_t0=t0, **kw)

    # -- updates
    def camera(self, F=None, M=None, outliers=0.15, outlier_px=400.0):
        """A batch on the model's state.  It is redrawn (the next seed) until, on that state, some but not all of its features
        pass the gate -- none of them with outliers = 1 -- and no verdict is within window30.MIN_MARGIN of its critical value."""
        import window30
        from msckf_amd import synth
        from oracle import msckf_oracle as oracle
        m = self.model
        F = int(self.rng.integers(20, 41)) if F is None else F
        M = min(m.N, 8 if M is None else M)
        for _ in range(50):
            self.draws += 1
            prob = synth.make_problem(m.N, F, M, seed=100000 + 1000 * self.seed + self.draws, P=np.array(m.P), poses=(np.array(m.cam_R), np.array(m.cam_t)),
                                      outlier_fraction=outliers, outlier_px=outlier_px, variable_tracks=True, min_track=2 if outliers < 1.0 else min(3, M),
                                      **state_args())
            prob = dataclasses.replace(prob, cam_R0=np.array(m.cam_R0), cam_t0=np.array(m.cam_t0))
            ref = oracle.update(prob, dense_noise=False)
            n_acc = int(ref["accepted"].sum())
            if (n_acc == 0 if outliers >= 1.0 else 0 < n_acc < F) and fp.gate_margin(ref) >= 10 * window30.MIN_MARGIN:
                break
        else:
            raise AssertionError((self.name, len(self.ops), "no batch met the gate's conditions"))
        rc = self.op("set_features", expect=0, prob=prob)
        self.fresh = True
        self.meta[-1]["outliers"] = outliers
        return rc

    def run(self, **kw):
        rc = self.op("run", **kw)
        if rc == 0 and self.fresh:
            out = self.ops[self.last_batch()][1]["prob"]
            frac = self.meta[self.last_batch()]["outliers"]
            self.meta[-1]["partial"] = 0.0 < frac < 1.0 and out.F >= 20
            self.meta[-1]["reject_all"] = frac >= 1.0
        return rc

    def last_batch(self):
        return max(i for i, (n, _) in enumerate(self.ops) if n == "set_features")

    def rows(self, kind, m=3, gate=None, **kw):
        """gate: None, "above" (applied) or "below" (rejected): the critical value beside the model's gamma."""
        H, r, R = rr.rows_on(np.array(self.model.P), kind, m, self.rng)
        crit = 0.0
        if gate is not None:
            gamma = rr.update(self.model.P, H, r, R)["gamma"]
            crit = float(gamma * (1 + rr.GATE_REL)) if gate == "above" else float(gamma * (1 - rr.GATE_REL))
        return self.op("run_rows", H=H, r=r, R=R, crit=crit, **kw)

    def fix(self, which, gate=None, **kw):
        """velocity_fix / position_fix / zero_velocity, sized as rows_ref's zupt and tpos cases."""
        m, c0 = self.model, 12 if which == "position_fix" else 6
        sig = np.sqrt(np.diag(m.P))[c0:c0 + 3]
        R = np.diag((0.5 * sig) ** 2) if which == "zero_velocity" else rr._full_noise(self.rng, sig, 0.5)
        R = (R + R.T) / 2
        z = np.zeros(3) if which == "zero_velocity" else m.nom["t" if c0 == 12 else "v"] + 0.7 * sig * self.rng.standard_normal(3)
        H = np.zeros((3, c0 + 3))
        H[:, c0:] = np.eye(3)
        crit = 0.0
        if gate is not None:
            gamma = rr.update(m.P, H, z - m.nom["t" if c0 == 12 else "v"], R)["gamma"]
            crit = float(gamma * (1 + rr.GATE_REL)) if gate == "above" else float(gamma * (1 - rr.GATE_REL))
        args = dict(R=R, crit=crit) if which == "zero_velocity" else dict(z=z, R=R, crit=crit)
        return self.op(which, **args, **kw)

    def not_spd_rows(self, **kw):
        """R indefinite: S = -I."""
        H, r, _ = rr.rows_on(np.array(self.model.P), "imu", 6, self.rng)
        Hd = rr.pad(H, self.model.d)
        S0 = Hd @ self.model.P @ Hd.T
        return self.op("run_rows", H=H, r=r, R=-(S0 + S0.T) / 2 - np.eye(6), crit=0.0, **kw)

    # -- the calls that are illegal in the current state: name -> (op name, arguments, code)
    def illegal_calls(self):
        m, out = self.model, {}
        d = m.d
        H, r, R = rr.rows_on(np.array(m.P), "imu", 3, np.random.default_rng(0))
        out["rows_too_wide"] = ("run_rows", dict(H=np.ones((2, d + 1)), r=np.zeros(2), R=np.eye(2), crit=0.0), fm.ERR_ARG)
        Ra = np.array(R)
        Ra[0, 1] = np.nextafter(Ra[0, 1], 1.0)
        out["rows_R_not_symmetric"] = ("run_rows", dict(H=H, r=r, R=Ra, crit=0.0), fm.ERR_ARG)
        out["remove_out_of_range"] = ("remove_clones", dict(slots=[m.N]), fm.ERR_ARG)
        out["imu_batch_empty"] = ("propagate_imu", dict(gyro=np.zeros((0, 3)), acc=np.zeros((0, 3)), dt=np.zeros(0)), fm.ERR_ARG)
        if m.N >= 1:
            out["remove_repeated_slot"] = ("remove_clones", dict(slots=[m.N - 1, 0, m.N - 1]), fm.ERR_ARG)
        else:
            out["set_poses_without_clones"] = ("set_poses", dict(cam_R=np.zeros((0, 3, 3)), cam_t=np.zeros((0, 3)), cam_R0=np.zeros((0, 3, 3)), cam_t0=np.zeros((0, 3))), fm.ERR_STATE)
        if m.N == self.max_clones:
            out["augment_imu_full"] = ("augment_imu", {}, fm.ERR_ARG)
            out["augment_full"] = ("augment", dict(J15=np.zeros((6, 15)), R=np.eye(3), t=np.zeros(3)), fm.ERR_ARG)
        if m.batch is None:
            out["run_without_batch"] = ("run", {}, fm.ERR_STATE)
        if m.last is None:
            for name in ("result",) + COMMITS:
                out[name + "_void"] = (name, {}, fm.ERR_STATE)
        elif m.last["injected"]:
            out["inject_twice"] = ("commit_inject", {}, fm.ERR_STATE)
        return out

    def refuse(self, which):
        name, kw, code = self.illegal_calls()[which]
        return self.op(name, expect=code, illegal=True, **kw)

    def sequence(self):
        return Sequence(self.name, self.max_clones, tuple(self.ops), tuple(self.meta))


# ---- the named sequences -----------------------------------------------------------------------------------------------------------

def _commit_paths():
    b = Builder("commit_paths", MAX_CLONES, 5, 1)
    for kind in ("camera", "rows"):
        def update():
            if kind == "camera":
                b.imu()
                b.camera()
                b.run(expect=0)
            else:
                b.rows("dense", 6, expect=0)
        update()                                         # commit without result
        b.op("commit_inject", expect=0)
        update()                                         # result then commit
        b.op("result", expect=0)
        b.op("commit_covariance", expect=0)
        update()                                         # result twice, covariance twice, injection once
        b.op("result", expect=0)
        b.op("result", expect=0)
        b.op("commit_covariance", expect=0)
        b.op("commit_covariance", expect=0)
        b.op("commit_inject", expect=0)
        b.op("covariance", expect=0)
        b.op("nominal", expect=0)
        update()                                         # commit_inject twice: the second is refused
        b.op("commit_inject", expect=0)
        b.op("nominal", expect=0)
        b.op("covariance", expect=0)
        b.refuse("inject_twice")
        b.op("commit_covariance", expect=0)              # ... and the covariance commit stays repeatable behind it
        b.op("nominal", expect=0)
        b.op("covariance", expect=0)
    return b.sequence()


def _void_results():
    b = Builder("void_results", MAX_CLONES, 4, 2)
    voiding = (lambda: b.host_propagate(expect=0), lambda: b.imu(expect=0), lambda: b.poses(expect=0), lambda: b.host_augment(expect=0),
               lambda: b.op("augment_imu", expect=0), lambda: b.op("remove_clones", expect=0, slots=[1]), lambda: b.reprior(4),
               lambda: b.camera())                       # (the next batch: the header asks to read and keep a run before it is loaded)
    for i, void in enumerate(voiding):
        if i % 2 == 0 and b.model.N >= 2:
            b.camera()
            b.run(expect=0)
        else:
            b.rows("imu", 3, expect=0)
        void()
        b.op("covariance", expect=0)
        b.op("nominal", expect=0)
        for name in ("result",) + COMMITS:
            b.op(name, expect=fm.ERR_STATE, illegal=True)
        b.op("covariance", expect=0)
        b.op("nominal", expect=0)
    b.rows("zupt", expect=0)                             # ... and the filter goes on
    b.op("commit_inject", expect=0)
    b.op("nominal", expect=0)
    return b.sequence()


def _batch_lifetime():
    b = Builder("batch_lifetime", MAX_CLONES, 6, 3)
    b.camera()
    b.rows("tpos", expect=0)
    b.op("commit_inject", expect=0)
    b.run(expect=0)                                      # the same batch on the new P and the new poses
    b.op("result")
    b.op("commit_inject")
    b.imu(expect=0)
    b.run(expect=0)                                      # ... behind a propagation
    b.op("result")
    b.op("augment_imu", expect=0)
    b.op("run", expect=fm.ERR_STATE, illegal=True)       # the batch went with the old layout
    b.op("covariance", expect=0)
    b.camera()
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.op("nominal", expect=0)
    b.op("covariance", expect=0)
    return b.sequence()


def _stale_mirror():
    b = Builder("stale_mirror", MAX_CLONES, 5, 4)
    b.imu()
    b.rows("clone", 6, expect=0)
    b.op("commit_inject", expect=0)                      # the device's poses lead the host's copy from here on
    b.op("remove_clones", expect=0, slots=[0, 3])
    b.host_augment(expect=0)
    b.imu()
    b.op("augment_imu", expect=0)
    b.camera()
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.poses(expect=0)                                    # overrides: poses and null poses of the caller
    b.camera()
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.op("remove_clones", expect=0, slots=[1])
    b.camera()
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("nominal", expect=0)                            # only now is the record read
    b.op("covariance", expect=0)
    return b.sequence()


def _mixed_propagation():
    b = Builder("mixed_propagation", MAX_CLONES, 3, 5)
    for i in range(3):
        b.host_propagate(expect=0)
        b.imu(expect=0)
    b.op("nominal", expect=0)
    b.op("covariance", expect=0)
    b.host_propagate(expect=0)
    b.imu(5, expect=0)
    b.fix("velocity_fix", expect=0)                      # behind a pending propagate_imu, nothing read back
    b.op("commit_inject", expect=0)
    b.imu(2, expect=0)
    b.host_propagate(expect=0)
    b.fix("position_fix", expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.imu(1, expect=0)
    b.fix("zero_velocity", expect=0)
    b.op("commit_inject", expect=0)
    b.op("nominal", expect=0)
    b.op("covariance", expect=0)
    return b.sequence()


def _refusals_between():
    b = Builder("refusals_between", 8, 6, 6)

    def sound(i):                                        # an accepted update that must come out right
        if i % 2:
            b.rows(("dense", "imu", "zupt")[i % 3], (17, 6, 3)[i % 3], expect=0)
        else:
            b.camera()
            b.run(expect=0)
        b.op("result", expect=0)
        b.op("commit_inject", expect=0)
        b.op("covariance", expect=0)
        b.op("nominal", expect=0)

    b.imu()
    b.rows("imu", 6, gate="below", expect=0)             # gated rows, rejected
    b.op("result", expect=fm.NOOP)
    b.op("commit_inject", expect=fm.NOOP)
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    sound(1)
    b.not_spd_rows(expect=0)                             # R indefinite
    b.op("result", expect=fm.ERR_NOT_SPD)
    b.op("commit_covariance", expect=fm.ERR_NOT_SPD)
    b.op("commit_inject", expect=fm.ERR_NOT_SPD)
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    sound(0)
    b.camera(outliers=1.0, outlier_px=2000.0)            # a camera batch that rejects every feature
    b.run(expect=0)
    b.op("result", expect=fm.NOOP)
    b.op("commit_inject", expect=fm.NOOP)
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    sound(3)
    b.refuse("rows_too_wide")
    b.refuse("remove_repeated_slot")
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    sound(2)
    b.imu()
    b.op("augment_imu", expect=0)
    b.imu()
    b.host_augment(expect=0)
    assert b.model.N == b.max_clones
    b.refuse("augment_full")
    b.refuse("augment_imu_full")
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    sound(4)
    return b.sequence()


def _grow_and_shrink():
    b = Builder("grow_and_shrink", MAX_CLONES, 0, 7)

    def update(k):
        if b.model.N >= 2 and k % 2 == 0:
            b.camera()
            b.run(expect=0)
        else:
            b.rows(("imu", "dense", "zupt", "tpos")[k % 4], (6, 17, 3, 3)[k % 4], expect=0)
        if k % 3 == 0:
            b.op("result", expect=0)
        b.op("commit_inject", expect=0)

    b.rows("imu", 17, expect=0)                          # N = 0: d = 15
    b.op("commit_inject", expect=0)
    for k in range(8):                                   # 0 -> 8: d crosses 16 (N = 1), 32 (N = 3) and 48 (N = 6)
        b.imu()
        b.op("augment_imu", expect=0)                    # (behind a pending result: the views are re-seated)
        if b.model.N in (1, 2, 3, 5, 6, 8):
            update(k)
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    b.op("remove_clones", expect=0, slots=[0])           # the first
    update(1)
    b.op("remove_clones", expect=0, slots=[b.model.N - 1])     # the last
    update(2)
    b.op("remove_clones", expect=0, slots=[4, 1, 2, 5])  # several at once: N = 2
    assert b.model.N == 2
    update(4)
    b.op("nominal", expect=0)
    for k in range(6):                                   # 2 -> 8
        b.imu()
        b.op("augment_imu", expect=0)
        if b.model.N in (3, 6, 8):
            update(k + 1)
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    return b.sequence()


def _reprior():
    b = Builder("reprior", MAX_CLONES, 6, 8)
    b.imu()
    b.camera()
    b.run(expect=0)
    b.op("commit_inject", expect=0)
    b.reprior(3, biases=True)                            # another N: the batch and the result go, the record is set again
    b.op("run", expect=fm.ERR_STATE, illegal=True)
    b.op("commit_inject", expect=fm.ERR_STATE, illegal=True)
    b.op("covariance", expect=0)
    b.op("nominal", expect=0)
    b.imu()
    b.op("augment_imu", expect=0)
    b.camera()
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    keep = b.model
    b.op("set_prior", expect=0, P=np.array(keep.P), cam_R=np.array(keep.cam_R), cam_t=np.array(keep.cam_t))    # the same N: the batch stays
    b.op("result", expect=fm.ERR_STATE, illegal=True)
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.rows("zupt", expect=0)
    b.op("commit_inject", expect=0)
    b.op("nominal", expect=0)
    b.op("covariance", expect=0)
    return b.sequence()


def _long_tracks():
    b = Builder("long_tracks", 20, 18, 9)
    b.imu()
    b.camera(F=40, M=18)
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.rows("dense", 17, expect=0)                        # rows between split camera updates
    b.op("commit_inject", expect=0)
    b.imu()
    b.op("augment_imu", expect=0)
    b.camera(F=40, M=19)
    b.run(expect=0)
    b.op("commit_inject", expect=0)                      # committed without result
    b.rows("clone", 6, expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.imu()
    b.op("augment_imu", expect=0)
    b.camera(F=40, M=20)
    b.run(expect=0)
    b.op("result", expect=0)
    b.op("commit_inject", expect=0)
    b.op("remove_clones", expect=0, slots=[0, 7])
    b.op("nominal", expect=0)
    b.op("covariance", expect=0)
    return b.sequence()


_NAMED = dict(commit_paths=_commit_paths, void_results=_void_results, batch_lifetime=_batch_lifetime, stale_mirror=_stale_mirror,
              mixed_propagation=_mixed_propagation, refusals_between=_refusals_between, grow_and_shrink=_grow_and_shrink,
              reprior=_reprior, long_tracks=_long_tracks)
NAMED = tuple(_NAMED)
RANDOM = tuple(f"random_{i:02d}" for i in range(N_RANDOM))
ALL = NAMED + RANDOM


# ---- the random sequences ----------------------------------------------------------------------------------------------------------

def _legal(b):
    m = b.model
    out = ["propagate_imu", "propagate", "run_rows", "velocity_fix", "position_fix", "zero_velocity", "covariance", "nominal"]
    if m.N < MAX_CLONES - 1:                             # N stays in 0 .. 8
        out += ["augment_imu", "augment"]
    if m.N >= 1:
        out += ["remove_clones", "set_poses"]
    if m.N >= 2:
        out.append("set_features")
    if m.batch is not None:
        out.append("run")
    if m.last is not None:
        out += ["result", "commit_covariance"]
        if not m.last["injected"]:
            out.append("commit_inject")
    return out


def _draw(b):
    rng, m = b.rng, b.model
    if rng.uniform() < ILLEGAL_RATE:
        calls = sorted(b.illegal_calls())
        return b.refuse(calls[int(rng.integers(len(calls)))])
    names = _legal(b)
    w = np.array([WEIGHTS[n] for n in names])
    name = names[int(rng.choice(len(names), p=w / w.sum()))]
    if name == "propagate_imu":
        return b.imu()
    if name == "propagate":
        return b.host_propagate()
    if name == "augment":
        return b.host_augment()
    if name == "remove_clones":
        n = int(rng.integers(1, min(3, m.N) + 1))
        return b.op("remove_clones", slots=[int(s) for s in rng.choice(m.N, n, replace=False)])
    if name == "set_poses":
        return b.poses()
    if name == "set_features":
        return b.camera()
    if name == "run":
        return b.run()
    if name == "run_rows":
        kinds = ["zupt", "pos", "tpos", "imu", "dense"] + (["clone"] if m.N >= 1 else [])
        kind = kinds[int(rng.integers(len(kinds)))]
        gate = (None, None, None, None, "above", "below")[int(rng.integers(6))]
        return b.rows(kind, int(ROWS_M[int(rng.integers(len(ROWS_M)))]), gate=gate)
    if name in ("velocity_fix", "position_fix", "zero_velocity"):
        return b.fix(name, gate=(None, None, "above", "below")[int(rng.integers(4))])
    return b.op(name)


def random_seed(i, k=None):
    name = RANDOM[i]
    return RANDOM_BASE + i + 1000 * (SEED_SKIPS.get(name, (0,))[0] if k is None else k)


def _random(i, k=None):
    seed = random_seed(i, k)
    b = Builder(RANDOM[i], MAX_CLONES, int(np.random.default_rng([seed, 1]).integers(0, 8)), seed)
    while len(b.ops) < 2 + RANDOM_OPS:                   # (behind set_prior and set_nominal)
        _draw(b)
    return b.sequence()


@functools.lru_cache(maxsize=None)
def sequence(name, k=None):
    """The sequence of that name, built once and shared: leave all of it unchanged."""
    if name in _NAMED:
        return _NAMED[name]()
    return _random(RANDOM.index(name), k)


# ---- what a sequence is made of ----------------------------------------------------------------------------------------------------

def composition(seq):
    """Counts over the ops of a sequence, from the codes the model returned."""
    c = dict(applied=0, rows=0, camera=0, n_changed_behind_update=0, commit_without_result=0, illegal=0, readbacks=0, ops=len(seq.ops))
    run_kind, fetched, committed, any_applied = None, False, False, False
    for (name, _), meta in zip(seq.ops, seq.meta):
        rc = meta["rc"]
        c["illegal"] += int(meta["illegal"])
        c["readbacks"] += int(name in READBACKS)
        if name in UPDATES and rc == 0:
            run_kind, fetched, committed = ("camera" if name == "run" else "rows"), False, False
        elif name == "result" and rc >= 0:
            fetched = True
        elif name in COMMITS and rc == 0 and not committed:
            committed, any_applied = True, True
            c["applied"] += 1
            c[run_kind] += 1
            c["commit_without_result"] += int(not fetched)
        elif name in ("augment", "augment_imu", "remove_clones") and rc == 0:
            c["n_changed_behind_update"] += int(any_applied)
        if name in MUTATING and name not in COMMITS and rc == 0:
            run_kind = None
    return c


MISS_CODE = dict(applied="a", rows="r", camera="c", n_changed="n", commit_without_result="b")


def composition_misses(seq):
    """The rules of a drawn sequence it does not meet (empty: all met)."""
    c = composition(seq)
    rules = dict(applied=c["applied"] >= 3, rows=c["rows"] >= 1, camera=c["camera"] >= 1, n_changed=c["n_changed_behind_update"] >= 1,
                 commit_without_result=c["commit_without_result"] >= 1)
    return [k for k, ok in rules.items() if not ok]
