"""Mixed call sequences on the resident filter (tests/call_sequences.py) against the host model (tests/filter_model.py).

The engine and the model run each sequence in lockstep; the model runs free and is never re-seeded from the device.  After every
op the return codes are compared (`EngineError.code` counts as the return) and `eng.n_clones` follows the model.  At every
read-back op of the sequence and at its end:

  result       status and the accepted mask exact (its shape too); dx and P_new in the five measures of filter_prior.metrics
               against the model below TOL = 1e-8, BASELINE.json's fp64 figure as tests/test_gpu_rows.py applies it
  covariance   rel_err and scaled_P below TOL (and update_term, against the prior the last commit replaced); bit-symmetric
  nominal      R, t, v, the biases, the null state and every clone pose within POSE_TOL = 1e-9
               (tests/test_gpu_filter_prior.py); rotations orthogonal to 1e-14.  The null poses of the clones have no reader in
               the ABI: they are held through the camera updates that linearise about them (`stale_mirror` gives them values
               of their own)
  unchanged    where the model's P, poses and record did not change since the last read of the same kind -- refused calls, void
               results, no-ops, runs that were not committed, a repeated commit_covariance -- the engine's are BITWISE what
               they were

Every sequence runs twice, on the same engine: as written, and with a full read-back (result where there is one, covariance,
nominal) behind every op.  The final covariance and nominal state of the two runs must be bitwise equal: reading a result or
refreshing the pose mirror must not change what the filter computes (k_rows.h, DESIGN 3.3: the same bits from the same
launches).  Each test prints one line, CALLSEQ <name> <worst e_dx e_P s_dx s_P u_P pose>."""
import numpy as np
import pytest

import call_sequences as cs
import filter_model as fm
import filter_prior as fp

pytestmark = pytest.mark.gpu

TOL = 1e-8              # BASELINE.json, fp64
POSE_TOL = 1e-9         # tests/test_gpu_filter_prior.py
ORTHOGONAL = 1e-14

_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def engine(max_clones):
    """One engine per window capacity, brought back to an empty window: no clone, no batch, no result."""
    from msckf_amd.api import UpdateEngine
    if max_clones not in _engines:
        _engines[max_clones] = UpdateEngine(max_clones=max_clones, max_features=64, max_track=max_clones)
    eng = _engines[max_clones]
    a = cs.state_args()
    eng.set_prior(np.array(fp.filter_prior(0)[0]), a["gravity"], a["K"], a["sigma"])
    return eng


def drive(eng, op):
    """One op on the engine: (code, payload), as call_sequences.step gives them for the model."""
    from msckf_amd import _ffi
    name, kw = op
    a = cs.state_args()
    gate = lambda: kw["crit"] if kw["crit"] > 0 else False
    try:
        if name == "set_prior":
            eng.set_prior(kw["P"], a["gravity"], a["K"], a["sigma"], kw["cam_R"], kw["cam_t"], kw.get("cam_R0"), kw.get("cam_t0"))
        elif name == "set_nominal":
            eng.set_nominal(kw["R"], kw["t"], kw["v"], a["gravity"], fp.head()["Qc"], T_I_C=cs.extrinsics(), b_g=kw.get("b_g"), b_a=kw.get("b_a"))
        elif name == "set_features":
            eng.set_features(kw["prob"])
        elif name == "run_rows":
            eng.run_rows(kw["H"], kw["r"], kw["R"], gate=gate())
        elif name in ("velocity_fix", "position_fix"):
            getattr(eng, name)(kw["z"], kw["R"], gate=gate())
        elif name == "zero_velocity":
            eng.zero_velocity(kw["R"], gate=gate())
        elif name == "result":
            res = eng.result()
            return res.status, dict(status=res.status, dx=res.dx, P_new=res.P_new, accepted=res.accepted)
        elif name in cs.COMMITS:
            return getattr(eng, name)(), None
        elif name == "covariance":
            return 0, eng.covariance()
        elif name == "nominal":
            return 0, eng.nominal()
        else:
            getattr(eng, name)(**kw)
    except _ffi.EngineError as e:
        return e.code, None
    return 0, None


def _state(m):
    _, nom = m.nominal()
    out = dict(P=m.P, cam_R=m.cam_R, cam_t=m.cam_t, cam_R0=m.cam_R0, cam_t0=m.cam_t0)
    out.update({} if nom is None else {k: nom[k] for k in fm.NOMINAL_KEYS})
    return {k: np.array(v) for k, v in out.items()}


class Lockstep:
    def __init__(self, seq, full):
        self.seq, self.full = seq, full
        self.eng, self.model = engine(seq.max_clones), fm.FilterModel(seq.max_clones)
        self.worst = np.zeros(6)
        self.cov = self.nom = None             # the engine's last reads, while the model says nothing changed since
        self.commit_prior = None               # the prior the last commit replaced, while P is that commit's
        self.split_updates = 0

    def note(self, e, where):
        e = np.asarray(e, dtype=np.float64)
        self.worst[:e.size] = np.maximum(self.worst[:e.size], e)
        assert e.max() < TOL, (self.seq.name, where, e)

    def check_result(self, i, got):
        run = self.model.last
        rc, want = self.model.result()
        assert got["status"] == rc and got["accepted"].shape == want["accepted"].shape, (self.seq.name, i)
        assert np.array_equal(got["accepted"], want["accepted"]), (self.seq.name, i)
        assert got["dx"].shape == (self.model.d,) and got["P_new"].shape == (self.model.d,) * 2
        assert np.array_equal(got["P_new"], got["P_new"].T), (self.seq.name, i)
        if rc == fm.OK:
            self.note(fp.metrics(got["dx"], got["P_new"], want, run["prior"]), (i, "result"))
        else:                                  # a no-op: dx = 0, P_out = the prior
            assert not got["dx"].any()
            self.note((0.0, fp.rel_err(got["P_new"], want["P_new"]), 0.0, fp.scaled_P(got["P_new"], want["P_new"])), (i, "no-op"))

    def check_covariance(self, i, P):
        want = self.model.P
        assert P.shape == want.shape and np.array_equal(P, P.T), (self.seq.name, i)
        u = fp.update_term(P, want, self.commit_prior) if self.commit_prior is not None else 0.0
        self.note((0.0, fp.rel_err(P, want), 0.0, fp.scaled_P(P, want), u), (i, "covariance"))
        if self.cov is not None:
            assert np.array_equal(P, self.cov), (self.seq.name, i, "the covariance moved where nothing was applied")
        self.cov = P

    def check_nominal(self, i, got):
        _, want = self.model.nominal()
        N = self.model.N
        assert got["cam_R"].shape == (N, 3, 3) and got["cam_t"].shape == (N, 3), (self.seq.name, i)
        gap = max(float(np.max(np.abs(got[k] - want[k]))) if want[k].size else 0.0 for k in want)
        self.worst[5] = max(self.worst[5], gap)
        assert gap <= POSE_TOL, (self.seq.name, i, gap, {k: float(np.max(np.abs(got[k] - want[k]))) for k in want if want[k].size})
        for R in (got["R"], got["R0"], *got["cam_R"]):
            assert np.max(np.abs(R.T @ R - np.eye(3))) < ORTHOGONAL, (self.seq.name, i)
        if self.nom is not None:
            assert all(np.array_equal(got[k], self.nom[k]) for k in got), (self.seq.name, i, "the nominal state moved where nothing was applied")
        self.nom = got

    def read(self, i, name):
        rc, got = drive(self.eng, (name, {}))
        want_rc = cs.step(self.model, (name, {}))[0]
        assert rc == want_rc, (self.seq.name, i, name, rc, want_rc)
        if got is not None:
            getattr(self, "check_" + name)(i, got)

    def run(self):
        eng, model = self.eng, self.model
        for i, (op, meta) in enumerate(zip(self.seq.ops, self.seq.meta)):
            name = op[0]
            if name in cs.READBACKS:
                self.read(i, name)
            else:
                before = _state(model) if model.P is not None else None
                want_rc, _ = cs.step(model, op)
                rc, _ = drive(eng, op)
                assert rc == want_rc == meta["rc"], (self.seq.name, i, name, rc, want_rc, meta["rc"])
                after = _state(model)
                loaded = rc == 0 and name in ("set_prior", "set_nominal", "set_poses")      # (the caller's values replace the engine's)
                if loaded or before is None or set(before) != set(after) or any(not np.array_equal(before[k], after[k]) for k in after):
                    self.cov = self.nom = None
                    self.commit_prior = model.last["prior"] if name in cs.COMMITS else None
                if name == "run" and rc == 0 and self.seq.name == "long_tracks":
                    self.split_updates += int(eng.debug_split()["long_tracks"] > 0)
            assert eng.n_clones == model.N, (self.seq.name, i, name)
            if self.full and i >= 1:           # (behind set_prior and set_nominal)
                if model.last is not None and model.last["rc"] >= 0:
                    self.read(i, "result")
                self.read(i, "covariance")
                self.read(i, "nominal")
        n = len(self.seq.ops)
        self.read(n, "covariance")
        self.read(n, "nominal")
        return self.cov, self.nom


@pytest.mark.parametrize("name", cs.ALL)
def test_sequence(name):
    seq = cs.sequence(name)
    plain = Lockstep(seq, full=False)
    P, nom = plain.run()
    full = Lockstep(seq, full=True)
    P_full, nom_full = full.run()
    worst = np.maximum(plain.worst, full.worst)
    print(f"CALLSEQ {name} " + " ".join(f"{x:.2e}" for x in worst))
    if name == "long_tracks":
        assert plain.split_updates >= 2, plain.split_updates
    assert np.array_equal(P, P_full), (name, "reading results changed the covariance", float(np.max(np.abs(P - P_full))))
    assert all(np.array_equal(nom[k], nom_full[k]) for k in nom), (name, "reading results changed the nominal state")
