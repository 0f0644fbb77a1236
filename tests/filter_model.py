"""A host model of the resident filter: what a context holds between calls and what every call of the resident path does to
it, as `include/msckf_mi355x.h` states it.  Host only, NumPy; not a conftest: imported by name.

The model is the contract, not the engine: it knows nothing of streams, mirrors or serial numbers.  Every arithmetic step is
a function the project already has --

  oracle.msckf_oracle       update, propagate_covariance, augment_covariance, remove_clones_covariance
  msckf_amd.propagation     imu_transition, augmentation
  nominal_ref               integrate
  rows_ref                  update (or update_chol: the other exact form, `rows_form`)
  msckf_amd.inject          inject_state

-- and the class only keeps the books: which P, which poses, which record, which batch, which run.  Methods carry the
engine's names (`msckf_amd.api.UpdateEngine`) and RETURN the engine's codes; where the engine's Python mirror raises
`EngineError`, the model returns the code.

  void results    propagate, propagate_imu, set_poses, augment, augment_imu, remove_clones and set_state void the last run:
                  result and both commits then return ERR_STATE and change nothing.  So does set_features: the gate results
                  of the old batch give way to the new one's, so a run is read and kept BEFORE the next batch is loaded
  batch lifetime  augment, augment_imu, remove_clones and a set_state with another N drop the loaded batch (run: ERR_STATE);
                  propagation, set_poses and a rows update leave it alone
  no-ops          a camera update with nothing accepted and a gated rows update return 1 from result and both commits
  not SPD         a rows run whose S has no Cholesky factor returns ERR_NOT_SPD from the readers; nothing changes
  injection       commit_covariance is repeatable; a run is injected once, the second commit_inject returns ERR_STATE
  a refused call  (an argument or call-order error) changes nothing at all, the last run included

`reverse_features` runs every camera batch with its features in reversed order (the accepted mask is put back): with
`rows_form="chol"` the second exact form of every update, for the reference spread of a call sequence
(tests/test_call_sequences.py)."""
import dataclasses
from types import SimpleNamespace

import numpy as np

import nominal_ref
import rows_ref as rr

OK, NOOP, ERR_ARG, ERR_NOT_SPD, ERR_STATE = 0, 1, -1, -4, -5
MAX_ROWS = 32                    # MSCKF_MAX_ROWS
IMU_BATCH_MAX = 64               # MSCKF_IMU_BATCH_MAX
FIX_COLUMN = {"position": 12, "velocity": 6}       # the error state is ordered theta, b_g, v, b_a, p

NOMINAL_KEYS = ("R", "t", "v", "b_g", "b_a", "R0", "t0", "v0")


def _f(a, shape=None):
    a = np.array(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


class FilterModel:
    def __init__(self, max_clones, rows_form="literal", reverse_features=False):
        self.max_clones = int(max_clones)
        self.rows_update = {"literal": rr.update, "chol": rr.update_chol}[rows_form]
        self.reverse_features = bool(reverse_features)
        self.P = None                              # (d, d); None: no state yet
        self.cam_R, self.cam_t = np.zeros((0, 3, 3)), np.zeros((0, 3))
        self.cam_R0, self.cam_t0 = np.zeros((0, 3, 3)), np.zeros((0, 3))
        self.gravity = self.K = self.sigma = None
        self.nom = None                            # the nominal record; None: no set_nominal yet
        self.batch = None                          # the loaded camera batch (an UpdateProblem; its state fields are not read)
        self.last = None                           # the last run; None: there is none, or it was voided
        self.P_before_commit = None                # the prior the last applied commit replaced (the update-term measure)

    # ---- what the engine reports about itself ----------------------------------------------------------------------------
    @property
    def N(self):
        return int(self.cam_R.shape[0])

    n_clones = N

    @property
    def d(self):
        return 15 + 6 * self.N

    def _void(self):
        self.last = None

    # ---- loading and priors ------------------------------------------------------------------------------------------------
    def set_state(self, P, gravity, K, sigma, cam_R=None, cam_t=None, cam_R0=None, cam_t0=None):
        P = _f(P)
        N = (P.shape[0] - 15) // 6
        if P.shape != (15 + 6 * N,) * 2 or N < 0 or N > self.max_clones:
            return ERR_ARG
        if self.P is None or N != self.N:
            self.batch = None
        self.P = P
        self.cam_R = _f(np.zeros((0, 3, 3)) if cam_R is None else cam_R, (N, 3, 3))
        self.cam_t = _f(np.zeros((0, 3)) if cam_t is None else cam_t, (N, 3))
        self.cam_R0 = self.cam_R.copy() if cam_R0 is None else _f(cam_R0, (N, 3, 3))
        self.cam_t0 = self.cam_t.copy() if cam_t0 is None else _f(cam_t0, (N, 3))
        self.gravity, self.K, self.sigma = _f(gravity), _f(K), float(sigma)
        self._void()
        return OK

    set_prior = set_state

    def set_nominal(self, R, t, v, gravity, noise, T_I_C, b_g=None, b_a=None, R0=None, t0=None, v0=None, planet_rate=None):
        if self.P is None:
            return ERR_STATE
        z3 = np.zeros(3)
        self.nom = dict(R=_f(R, (3, 3)), t=_f(t), v=_f(v), b_g=_f(z3 if b_g is None else b_g), b_a=_f(z3 if b_a is None else b_a),
                        R0=_f(R if R0 is None else R0, (3, 3)), t0=_f(t if t0 is None else t0), v0=_f(v if v0 is None else v0),
                        gravity=_f(gravity), planet_rate=_f(z3 if planet_rate is None else planet_rate), Qc=_f(noise, (12, 12)),
                        T_I_C=(_f(T_I_C[0], (3, 3)), _f(T_I_C[1])),
                        alias=False)               # the null state moves with the state once propagate_imu has run
        return OK

    def set_poses(self, cam_R, cam_t, cam_R0=None, cam_t0=None):
        if self.P is None or self.N < 1:
            return ERR_STATE
        N = self.N
        self.cam_R, self.cam_t = _f(cam_R, (N, 3, 3)), _f(cam_t, (N, 3))
        self.cam_R0 = self.cam_R.copy() if cam_R0 is None else _f(cam_R0, (N, 3, 3))
        self.cam_t0 = self.cam_t.copy() if cam_t0 is None else _f(cam_t0, (N, 3))
        self._void()
        return OK

    def set_features(self, prob):
        """The batch of `prob` (its tracks and inverse-depth points; P and the poses of `prob` are not read)."""
        if self.P is None:
            return ERR_STATE
        self.batch = None                          # the previous batch is gone from here on, and the run that read it with it
        self._void()
        slots = np.asarray(prob.obs_slot).reshape(-1)
        if prob.F and (slots.min() < 0 or slots.max() >= self.N):
            return ERR_ARG
        self.batch = prob
        return OK

    # ---- propagation and clones --------------------------------------------------------------------------------------------
    def propagate(self, Phi, Q):
        from oracle import msckf_oracle as oracle
        if self.P is None:
            return ERR_STATE
        self.P = oracle.propagate_covariance(self.P, _f(Phi, (15, 15)), _f(Q, (15, 15)))
        self._void()
        return OK

    def propagate_imu(self, gyro, acc, dt):
        from msckf_amd import propagation
        from oracle import msckf_oracle as oracle
        if self.nom is None:
            return ERR_STATE
        gyro, acc, dt = _f(gyro).reshape(-1, 3), _f(acc).reshape(-1, 3), _f(dt).reshape(-1)
        if not 1 <= dt.size <= IMU_BATCH_MAX:
            return ERR_ARG
        s = self.nom
        for k in range(dt.size):
            g, a = gyro[k] - s["b_g"], acc[k] - s["b_a"]                         # MSCKF.py:166-167
            R0, t0, v0 = s["R0"], s["t0"], s["v0"]
            R, t, v, _ = nominal_ref.integrate(s["R"], s["t"], s["v"], a, g, float(dt[k]), s["gravity"], s["planet_rate"])
            Phi, Q = propagation.imu_transition(R, t, v, R0, t0, v0, g, a, float(dt[k]), s["gravity"], s["Qc"], s["planet_rate"])
            self.P = oracle.propagate_covariance(self.P, Phi, Q)
            s.update(R=R, t=t, v=v, R0=R.copy(), t0=t.copy(), v0=v.copy(), alias=True)      # :247-248
        self._void()
        return OK

    def _append_clone(self, J, R, t):
        from oracle import msckf_oracle as oracle
        self.P = oracle.augment_covariance(self.P, J)
        R, t = _f(R, (1, 3, 3)), _f(t, (1, 3))
        self.cam_R, self.cam_t = np.concatenate([self.cam_R, R]), np.concatenate([self.cam_t, t])
        self.cam_R0, self.cam_t0 = np.concatenate([self.cam_R0, R]), np.concatenate([self.cam_t0, t])     # Camera.py:11
        self.batch = None
        self._void()
        return OK

    def augment(self, J15, R, t):
        if self.P is None:
            return ERR_STATE
        if self.N + 1 > self.max_clones:
            return ERR_ARG
        return self._append_clone(_f(J15, (6, 15)), R, t)

    def augment_imu(self):
        from msckf_amd import propagation
        if self.nom is None:
            return ERR_STATE
        if self.N + 1 > self.max_clones:
            return ERR_ARG
        # T_W_I = identity makes propagation.augmentation's T_W_I^-1 T_W_C the record's extrinsics themselves
        J, R, t = propagation.augmentation(self.nom["R"], self.nom["t"], (np.eye(3), np.zeros(3)), self.nom["T_I_C"])
        return self._append_clone(J, R, t)

    def remove_clones(self, slots):
        from oracle import msckf_oracle as oracle
        slots = [int(s) for s in np.asarray(slots).reshape(-1)]
        if self.P is None:
            return ERR_STATE
        if any(s < 0 or s >= self.N for s in slots) or len(set(slots)) != len(slots):
            return ERR_ARG
        if not slots:
            return OK
        self.P = oracle.remove_clones_covariance(self.P, slots)
        keep = [s for s in range(self.N) if s not in slots]
        self.cam_R, self.cam_t, self.cam_R0, self.cam_t0 = self.cam_R[keep], self.cam_t[keep], self.cam_R0[keep], self.cam_t0[keep]
        self.batch = None
        self._void()
        return OK

    # ---- runs ----------------------------------------------------------------------------------------------------------------
    def problem(self):
        """The loaded batch on the current P and poses."""
        return dataclasses.replace(self.batch, P=self.P, cam_R=self.cam_R, cam_t=self.cam_t, cam_R0=self.cam_R0, cam_t0=self.cam_t0,
                                   gravity=self.gravity, K=self.K, sigma=self.sigma)

    def run(self):
        from oracle import msckf_oracle as oracle
        if self.P is None or self.batch is None:
            return ERR_STATE
        prob = self.problem()
        F = prob.F
        if self.reverse_features:
            order = np.arange(F)[::-1]
            out = oracle.update(prob.take(order), dense_noise=False)
            back = lambda a: np.asarray(a)[np.argsort(order)]
            out.update(accepted=back(out["accepted"]), gamma=back(out["gamma"]), crit=back(out["crit"]))
        else:
            out = oracle.update(prob, dense_noise=False)
        self.last = dict(kind="camera", rc=int(out["status"]), dx=out["dx"], P_new=out["P_new"], accepted=np.asarray(out["accepted"], dtype=np.uint8),
                         gamma=out["gamma"], crit=out["crit"], prior=self.P, injected=False)
        return OK

    def run_rows(self, H, r, R, crit=0.0):
        """`crit` > 0 gates at that value (the engine's `gate=`), else the update is not gated."""
        if self.P is None:
            return ERR_STATE
        H = np.atleast_2d(_f(H))
        r, R = _f(r).reshape(-1), _f(R)
        m, n_cols = (H.shape if H.size else (0, 0))
        if not (1 <= m <= MAX_ROWS and 1 <= n_cols <= self.d) or r.size != m or R.shape != (m, m) or not np.array_equal(R, R.T):
            return ERR_ARG
        return self._rows(H, r, R, crit)

    def _rows(self, H, r, R, crit):
        Hd = rr.pad(H, self.d)
        S = Hd @ self.P @ Hd.T + R
        try:                                       # a pivot of S that is not a positive normal number
            spd = bool(np.all(np.isfinite(S))) and bool(np.all(np.isfinite(np.linalg.cholesky((S + S.T) / 2))))
        except np.linalg.LinAlgError:
            spd = False
        if not spd:
            self.last = dict(kind="rows", rc=ERR_NOT_SPD, prior=self.P, injected=False, gamma=np.nan)
            return OK
        out = self.rows_update(self.P, H, r, R, float(crit) if crit and crit > 0 else np.inf)
        self.last = dict(kind="rows", rc=int(out["status"]), dx=out["dx"], P_new=out["P_new"], accepted=np.array([out["applied"]], dtype=np.uint8),
                         gamma=out["gamma"], crit=float(crit) if crit and crit > 0 else np.inf, prior=self.P, injected=False)
        return OK

    def _fix(self, which, z, R, crit):
        if self.P is None or self.nom is None:
            return ERR_STATE
        z, R = _f(z).reshape(-1), _f(R)
        if z.size != 3 or R.shape != (3, 3) or not np.array_equal(R, R.T):
            return ERR_ARG
        c0 = FIX_COLUMN[which]
        H = np.zeros((3, c0 + 3))
        H[:, c0:] = np.eye(3)
        return self._rows(H, z - self.nom["t" if which == "position" else "v"], R, crit)     # r = z - h(nominal)

    def velocity_fix(self, z, R, crit=0.0):
        return self._fix("velocity", z, R, crit)

    def position_fix(self, z, R, crit=0.0):
        return self._fix("position", z, R, crit)

    def zero_velocity(self, R, crit=0.0):
        return self._fix("velocity", np.zeros(3), R, crit)

    # ---- reading and keeping -------------------------------------------------------------------------------------------------
    def result(self):
        """(code, dict(status, dx, P_new, accepted) or None when the code is an error)."""
        if self.last is None:
            return ERR_STATE, None
        run = self.last
        if run["rc"] < 0:
            return run["rc"], None
        return run["rc"], dict(status=run["rc"], dx=np.array(run["dx"]), P_new=np.array(run["P_new"]), accepted=np.array(run["accepted"]))

    def commit_covariance(self):
        if self.last is None:
            return ERR_STATE
        if self.last["rc"] != OK:
            return self.last["rc"]
        if self.P is not self.last["P_new"]:
            self.P_before_commit = self.last["prior"]
        self.P = self.last["P_new"]
        return OK

    def commit_inject(self):
        from msckf_amd import inject
        if self.nom is None or self.last is None:
            return ERR_STATE
        if self.last["injected"]:                  # a run is injected once
            return ERR_STATE
        rc = self.commit_covariance()
        if rc != OK:
            return rc
        s = self.nom
        pose = lambda R, t: SimpleNamespace(R=np.array(R), t=np.array(t))
        imu = SimpleNamespace(T_W_Ii=pose(s["R"], s["t"]), v_W_Ii=np.array(s["v"]), gyroscope_bias=np.array(s["b_g"]),
                              accelerometer_bias=np.array(s["b_a"]))
        cams = {i: SimpleNamespace(T_W_Ci=pose(self.cam_R[i], self.cam_t[i])) for i in range(self.N)}
        inject.inject_state(SimpleNamespace(imu=imu, cameras=cams), self.last["dx"])
        s.update(R=imu.T_W_Ii.R, t=imu.T_W_Ii.t, v=imu.v_W_Ii, b_g=imu.gyroscope_bias, b_a=imu.accelerometer_bias)
        if s["alias"]:
            s.update(R0=s["R"].copy(), t0=s["t"].copy(), v0=s["v"].copy())
        self.cam_R = np.array([cams[i].T_W_Ci.R for i in range(self.N)]).reshape(self.N, 3, 3)
        self.cam_t = np.array([cams[i].T_W_Ci.t for i in range(self.N)]).reshape(self.N, 3)
        self.cam_R0, self.cam_t0 = self.cam_R.copy(), self.cam_t.copy()          # a clone's null pose is its pose (Camera.py:10-11)
        self.last["injected"] = True
        return OK

    def covariance(self):
        if self.P is None:
            return ERR_STATE, None
        return OK, np.array(self.P)

    def nominal(self):
        if self.nom is None:
            return ERR_STATE, None
        out = {k: np.array(self.nom[k]) for k in NOMINAL_KEYS}
        out["cam_R"], out["cam_t"] = np.array(self.cam_R), np.array(self.cam_t)
        return OK, out
