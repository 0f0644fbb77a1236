"""The host model of the resident filter (`filter_model.FilterModel`) and the table of call sequences (`call_sequences`) are
themselves held to something, on the CPU:

1  the model replays the reference's recorded runs -- the 30-clone run `golden/window30/seq_window30.npz` with the nominal state
   in the model (propagate_imu, augment_imu, commit_inject), `seq_short` in the host form (propagate, augment, set_poses) -- and
   stays on the fixtures' checkpoints, probes, dx and poses at the tolerances tests/test_window30.py holds the oracle to;
2  every sequence meets its conditions: each applied update removes at least rows_ref.MIN_UPDATE of |P|, each gate verdict is
   at least window30.MIN_MARGIN from its critical value, a partial camera update accepts some but not all, a drawn sequence
   meets `call_sequences.composition_misses`;
3  the spread: a second model with the project's other exact forms (rows_ref.update_chol; the camera batch in reversed order)
   runs each sequence free beside the first; at every read-back and at the end the two agree within 1e-10 in the measures of
   filter_prior.metrics and 1e-11 on the poses and the nominal state -- a hundred times under the GPU test's bounds.  A sequence
   that misses is ill-conditioned and is replaced by the seed rule (call_sequences.SEED_SKIPS)."""
import numpy as np
import pytest

import call_sequences as cs
import filter_model as fm
import filter_prior as fp
import nominal_ref
import rows_ref as rr
import window30
from conftest import load_sequence, rel_err
from test_window30 import DX_TOL, PROBE_TOL
from window30 import AUGMENT, PROCESS, PRUNE, REMOVE

SPREAD_TOL = 1e-10
SPREAD_POSE_TOL = 1e-11
POSE_TOL = 1e-9                  # tests/test_window30.py's bound on the poses after an injection


# ---- 1: the model against the reference's recorded runs ---------------------------------------------------------------------------

def test_model_carries_the_window30_run():
    from msckf_amd import propagation
    from oracle import msckf_oracle as oracle
    run = window30.Run()
    z = run.z
    params = run.select_params()
    gyro, acc = nominal_ref.raw_samples(run)
    m = fm.FilterModel(31)
    assert m.set_prior(z["P0"], z["gravity"], z["K"], run.sigma) == 0
    T_I_C = propagation.extrinsics((z["T_W_I_R"], z["T_W_I_t"]), (z["T_W_C_R"], z["T_W_C_t"]))
    assert m.set_nominal(z["imu_R0"][0], z["imu_t0"][0], z["imu_v0"][0], z["gravity"], z["Qc"], T_I_C) == 0
    keys, updates = [], 0
    worst = dict(dx=0.0, probe=0.0, pose=0.0)

    def close(a, b):
        e = float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.size(b) else 0.0
        worst["pose"] = max(worst["pose"], e)
        assert np.shape(a) == np.shape(b) and e <= POSE_TOL, e

    for kind, idx, o in nominal_ref.imu_groups(run):
        if kind == "imu":
            assert m.propagate_imu(gyro[idx], acc[idx], z["imu_dt"][idx]) == 0
            _, s = m.nominal()
            for name in ("R", "t", "v"):
                close(s[name], z["imu_" + name][idx[-1]])
                assert np.array_equal(s[name + "0"], s[name])                    # MSCKF.py:247-248
        elif kind == AUGMENT:
            a = run.aug(idx)
            assert m.augment_imu() == 0
            keys.append(int(a["key"]))
            close(m.cam_R[-1], a["cam_R"]), close(m.cam_t[-1], a["cam_t"])
        elif kind in (PROCESS, PRUNE):
            c = run.call(idx)
            assert c["keys"].tolist() == keys and m.n_clones == len(keys)
            prob = run.problem(c, m.P, m.cam_R, m.cam_t)
            sel = oracle.select_features(prob, run.tracks(c), params)
            assert np.array_equal(sel["flags"], c["flags"])
            valid = np.nonzero(c["flags"] & 1)[0]
            if len(valid):
                upd = prob.take(valid)
                upd.idp_m, upd.idp_rho = sel["idp_m"][valid], sel["idp_rho"][valid]
                assert m.set_features(upd) == 0 and m.run() == 0
                rc, res = m.result()
                assert rc == c["status"] and np.array_equal(res["accepted"], c["accepted"][valid])
                if rc == 0:
                    updates += 1
                    e = rel_err(res["dx"], c["dx"])
                    worst["dx"] = max(worst["dx"], e)
                    assert e < DX_TOL, (o, e)
                assert m.commit_inject() == rc
                assert m.commit_inject() == (fm.ERR_STATE if rc == 0 else rc)     # a run is injected once
            else:
                assert c["status"] == 1
            if kind == PRUNE:
                assert m.remove_clones(c["rm"]) == 0
                keys = [k for s, k in enumerate(keys) if s not in c["rm"]]
            close(m.cam_R, c["post_R"]), close(m.cam_t, c["post_t"])
        elif kind == REMOVE:
            c = run.call(idx)
            assert m.remove_clones(c["rm"]) == 0
            keys = [k for s, k in enumerate(keys) if s not in c["rm"]]
        assert m.n_clones == len(keys) == run.n_clones_after()[o]
        _, P = m.covariance()
        if o in run.probes:
            e = rel_err(P @ run.V[:P.shape[0]], run.probes[o])
            worst["probe"] = max(worst["probe"], e)
            assert e < PROBE_TOL, (o, kind, e)
        if o in run.checkpoints:
            assert rel_err(P, run.checkpoints[o]) < PROBE_TOL
    assert updates >= 10
    print(f"CALLSEQ model window30: {updates} updates, worst dx {worst['dx']:.2e} probes {worst['probe']:.2e} poses {worst['pose']:.2e}")


def test_model_carries_seq_short():
    from msckf_amd import propagation, synth
    head, ops = load_sequence("seq_short")
    m = fm.FilterModel(8)
    assert m.set_prior(head["P0"], head["gravity"], head["K"], float(head["sigma"])) == 0
    assert m.result()[0] == m.commit_covariance() == m.run() == fm.ERR_STATE
    worst = 0.0
    for op in ops:
        if op["kind"] == 0:
            Phi, Q = propagation.imu_transition(op["R"], op["t"], op["v"], op["R0"], op["t0"], op["v0"], op["gyro"], op["acc"],
                                                float(op["dt"]), head["gravity"], head["Qc"], op["w_planet"])
            assert m.propagate(Phi, Q) == 0
        elif op["kind"] == 1:
            J, cR, ct = propagation.augmentation(op["imu_R"], op["imu_t"], (head["T_W_I_R"], head["T_W_I_t"]), (head["T_W_C_R"], head["T_W_C_t"]))
            assert m.augment(J, cR, ct) == 0
            assert m.run() == fm.ERR_STATE                                       # the clone set changed: no batch
        elif op["kind"] == 2:
            N = op["cam_R"].shape[0]
            assert m.n_clones == N
            np.testing.assert_allclose(m.cam_R, op["cam_R"], atol=1e-12), np.testing.assert_allclose(m.cam_t, op["cam_t"], atol=1e-12)
            feats = synth.UpdateProblem(P=np.zeros((15 + 6 * N,) * 2), cam_R=op["cam_R"], cam_t=op["cam_t"], cam_R0=op["cam_R"], cam_t0=op["cam_t"],
                                        gravity=head["gravity"], K=head["K"], sigma=float(head["sigma"]), view_ptr=op["view_ptr"],
                                        obs_uv=op["obs_uv"], obs_slot=op["obs_slot"], idp_base=op["idp_base"], idp_m=op["idp_m"], idp_rho=op["idp_rho"])
            assert m.set_features(feats) == 0 and m.run() == 0
            rc, res = m.result()
            assert rc == int(op["status"]) and rel_err(res["dx"], op["dx"]) < DX_TOL
            assert m.commit_covariance() == rc == m.commit_covariance()          # repeatable
            assert m.set_poses(op["post_cam_R"], op["post_cam_t"]) == 0
            assert m.result()[0] == fm.ERR_STATE
        else:
            assert m.remove_clones(op["slots"]) == 0
        _, P = m.covariance()
        assert P.shape == op["P_after"].shape
        e = rel_err(P, op["P_after"])
        worst = max(worst, e)
        assert e < PROBE_TOL, (op["kind"], e)
    print(f"CALLSEQ model seq_short: worst P {worst:.2e}")


# ---- 2 and 3: every sequence ----------------------------------------------------------------------------------------------------------

def _snapshot(m):
    _, nom = m.nominal()
    return dict(P=np.array(m.P), cam_R=np.array(m.cam_R), cam_t=np.array(m.cam_t), cam_R0=np.array(m.cam_R0), cam_t0=np.array(m.cam_t0),
                **({} if nom is None else {k: nom[k] for k in fm.NOMINAL_KEYS}))


def _pose_gap(a, b):
    return max(float(np.max(np.abs(a[k] - b[k]))) if a[k].size else 0.0 for k in a if k != "P")


def conditions_and_spread(seq):
    """Steps the sequence on the model and on the model of the other exact forms.  Returns (what the sequence misses: a list of
    strings, the worst spread over the five measures and the poses)."""
    a, b = fm.FilterModel(seq.max_clones), fm.FilterModel(seq.max_clones, rows_form="chol", reverse_features=True)
    misses, worst, worst_pose = [], np.zeros(5), 0.0
    committed = False

    def spread_now(i, what, e):
        nonlocal worst
        worst = np.maximum(worst, e)
        if max(e) > SPREAD_TOL:
            misses.append(f"op {i} {what}: spread {max(e):.1e}")

    for i, (op, meta) in enumerate(zip(seq.ops, seq.meta)):
        name = op[0]
        before = _snapshot(a) if a.P is not None else None
        rc, got = cs.step(a, op)
        rc_b, got_b = cs.step(b, op)
        assert rc == rc_b == meta["rc"], (seq.name, i, name, rc, rc_b, meta["rc"])
        if (meta["illegal"] or (name in cs.COMMITS and rc != 0)) and before is not None:
            after = _snapshot(a)
            assert all(np.array_equal(before[k], after[k]) for k in before), (seq.name, i, name)      # refused: nothing changed
        run = a.last
        if name in cs.UPDATES and rc == 0:
            committed = False
            if run["rc"] >= 0:
                g, crit = np.atleast_1d(run["gamma"]), np.atleast_1d(run["crit"])
                gated = np.isfinite(crit)
                if gated.any() and float(np.min(np.abs(g[gated] - crit[gated]) / crit[gated])) < window30.MIN_MARGIN:
                    misses.append(f"op {i} {name}: a verdict within {window30.MIN_MARGIN} of its critical value")
                if b.last["rc"] != run["rc"] or not np.array_equal(b.last["accepted"], run["accepted"]):
                    misses.append(f"op {i} {name}: the two forms disagree on a verdict")
            n_acc = int(run["accepted"].sum()) if run["rc"] >= 0 else 0
            if meta["partial"] and not 0 < n_acc < run["accepted"].size:
                misses.append(f"op {i} run: meant to be partial, accepted {n_acc} of {run['accepted'].size}")
            if meta["reject_all"] and n_acc != 0:
                misses.append(f"op {i} run: meant to reject every feature, accepted {n_acc}")
        if name in cs.COMMITS and rc == 0 and not committed:
            committed = True
            removed = float(np.linalg.norm(run["prior"] - run["P_new"]) / np.linalg.norm(run["prior"]))
            if removed < rr.MIN_UPDATE:
                misses.append(f"op {i} {name}: the update removes {removed:.1e} of |P|")
        if name == "result" and rc == 0:
            spread_now(i, name, fp.metrics(got_b["dx"], got_b["P_new"], got, run["prior"]))
        last = i == len(seq.ops) - 1
        if name == "covariance" or last:
            spread_now(i, "covariance", (0.0, rel_err(b.P, a.P), 0.0, fp.scaled_P(b.P, a.P), 0.0))
        if name == "nominal" or last:
            gap = _pose_gap(_snapshot(a), _snapshot(b))
            worst_pose = max(worst_pose, gap)
            if gap > SPREAD_POSE_TOL:
                misses.append(f"op {i} nominal: spread {gap:.1e}")
    if seq.name in cs.RANDOM:
        misses += ["composition: " + r for r in cs.composition_misses(seq)]
    return misses, tuple(float(x) for x in worst) + (worst_pose,)


@pytest.mark.parametrize("name", cs.ALL)
def test_conditions_and_spread(name):
    seq = cs.sequence(name)
    misses, worst = conditions_and_spread(seq)
    print(f"CALLSEQ spread {name} " + " ".join(f"{x:.2e}" for x in worst))
    assert not misses, misses


def test_composition_of_the_table():
    assert len(cs.RANDOM) == 24 and len(set(cs.ALL)) == len(cs.ALL)
    for name in cs.NAMED:
        assert 8 <= len(cs.sequence(name).ops), name
    illegal = readbacks = ops = 0
    for name in cs.RANDOM:
        seq = cs.sequence(name)
        c = cs.composition(seq)
        assert c["ops"] == 2 + cs.RANDOM_OPS                                     # set_prior, set_nominal and the drawn ones
        illegal, readbacks, ops = illegal + c["illegal"], readbacks + c["readbacks"], ops + cs.RANDOM_OPS
    assert 0.12 <= illegal / ops <= 0.22, illegal / ops                         # about one in six
    assert 0.14 <= readbacks / ops <= 0.28, readbacks / ops                     # about one in five
    # the sizes: N in 0 .. 8 on the contexts of 9, the long tracks at 18 .. 20
    long_updates = 0
    seq = cs.sequence("long_tracks")
    for (name, kw) in seq.ops:
        if name == "set_features":
            prob = kw["prob"]
            span = np.diff(prob.view_ptr)
            assert 18 <= prob.N <= 20
            long_updates += int((span > 10).any())
    assert long_updates >= 2


def _miss_word(seq):
    """What a drawn sequence misses, in call_sequences.SEED_SKIPS' letters (the conditions only where the rules are met)."""
    misses = ["composition: " + r for r in cs.composition_misses(seq)] or conditions_and_spread(seq)[0]
    word = ""
    for m in misses:
        ch = cs.MISS_CODE.get(m.replace("composition: ", ""), "w" if "removes" in m else "s" if "spread" in m else "?")
        word += ch if ch not in word else ""
    return word


def test_seed_skips_are_explained():
    """Every entry names the first k that passes and, seed by seed, what the earlier ones missed; they do miss exactly that."""
    for name, (k, why) in cs.SEED_SKIPS.items():
        assert name in cs.RANDOM and k >= 1 and len(why.split()) == k, name
        for j, word in enumerate(why.split()):
            assert _miss_word(cs._random(cs.RANDOM.index(name), j)) == word, (name, j)
