#!/usr/bin/env python3
"""A direct measurement on the resident filter, two ways, at N clones (default 30 and 50), with a propagate_imu pending:

  (a) the path a caller had before msckf_run_rows: get_covariance + get_nominal, the update (MSCKF.py:604-614 in NumPy) and the
      injection on the host, import_covariance + set_nominal.  With --parent-lib it runs on that build of the library (an engine
      of its own), so the comparison is against the parent and not against the code under test.
  (b) zero_velocity + commit_inject, and run_rows with 32 dense rows + commit_inject.

Both are timed on the host clock from the call behind the pending propagate_imu to the point where the next propagate_imu
could be issued; (a), (b) and (b') alternate, every figure is the median over --reps rounds after --warmup.  The device time of
a rows run (the upload of H | r | R and the two launches) comes from HIP events on the engine's stream, per (m, n_cols).
Prints one markdown table per N and one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msckf_amd  # noqa: F401,E402
from msckf_amd import _ffi, inject, synth  # noqa: E402
from msckf_amd.api import UpdateEngine  # noqa: E402


def parent_engine(path, **kw):
    """An UpdateEngine on another build of the library (the symbols it shares with this one)."""
    cur = _ffi.load()
    lib = C.CDLL(path)
    for s in _ffi.SYMBOLS:
        if hasattr(lib, s):
            getattr(lib, s).argtypes, getattr(lib, s).restype = getattr(cur, s).argtypes, getattr(cur, s).restype
    orig = _ffi.load
    _ffi.load = lambda: lib
    try:
        return UpdateEngine(**kw)
    finally:
        _ffi.load = orig


class Events:
    """Two HIP events on the engine's stream."""

    def __init__(self, eng):
        self.hip = None
        for name in ("libamdhip64.so", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
            try:
                self.hip = C.CDLL(name)
                break
            except OSError:
                continue
        if self.hip is None:
            raise RuntimeError("libamdhip64.so not found")
        vp = C.c_void_p
        self.hip.hipEventCreate.argtypes = [C.POINTER(vp)]
        self.hip.hipEventRecord.argtypes = [vp, vp]
        self.hip.hipEventSynchronize.argtypes = [vp]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        self.stream = C.c_void_p(eng._lib.msckf_stream(eng._h))
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def record(self, i):
        assert self.hip.hipEventRecord(self.ev[i], self.stream) == 0

    def elapsed_us(self):
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value * 1000.0


def host_update(P, H, r, R):
    """MSCKF.py:604-614 with the caller's H (padded to d columns), r, R."""
    S = H @ P @ H.T + R
    K = P @ H.T @ np.linalg.inv(S)
    A = np.eye(P.shape[0]) - K @ H
    Pn = A @ P @ A.T + K @ R @ K.T
    return K @ r, (Pn + Pn.T) / 2


def setup(eng, prob, rng):
    eng.set_state(prob)
    eng._F = 0
    eng.set_nominal(np.eye(3), np.zeros(3), 0.05 * rng.standard_normal(3), prob.gravity, 1e-4 * np.eye(12),
                    T_I_C=(np.eye(3), np.zeros(3)))


def bench(N, reps, warmup, parent_lib):
    rng = np.random.default_rng(N)
    prob = synth.make_problem(N, 8, min(N, 4), seed=N)
    d = prob.d
    kw = dict(max_clones=N, max_features=16, max_track=8)
    eng_a = parent_engine(parent_lib, **kw) if parent_lib else UpdateEngine(**kw)
    eng_b = UpdateEngine(**kw)
    for e in (eng_a, eng_b):
        setup(e, prob, rng)
    s = np.sqrt(np.diag(prob.P))
    sig_v = 0.5 * s[6:9]
    Hz = np.zeros((3, d))
    Hz[:, 6:9] = np.eye(3)
    Rz = np.diag(sig_v ** 2)
    Hd = rng.standard_normal((32, d)) / s[None, :]
    Rd = np.diag(np.einsum("ij,jk,ik->i", Hd, prob.P, Hd) * rng.uniform(0.25, 4.0, 32))
    gyro, acc, dt = 0.01 * rng.standard_normal((4, 3)), np.tile(prob.gravity, (4, 1)) + 0.01 * rng.standard_normal((4, 3)), np.full(4, 0.005)
    P_buf, nom = np.zeros((d, d)), _ffi.NominalC()
    cam_R, cam_t = np.zeros((N, 3, 3)), np.zeros((N, 3))
    la, ha = eng_a._lib, eng_a._h

    def path_a():
        eng_a.propagate_imu(gyro, acc, dt)
        t0 = time.perf_counter()
        assert la.msckf_get_covariance(ha, _ffi.dptr(P_buf), None) == 0
        assert la.msckf_get_nominal(ha, C.byref(nom), _ffi.dptr(cam_R), _ffi.dptr(cam_t)) == 0
        v = np.array(nom.v)
        dx, Pn = host_update(P_buf, Hz, -v, Rz)                        # r = z - v, z = 0
        nom.R = (C.c_double * 9)(*inject.corrected_rotation(np.array(nom.R).reshape(3, 3), dx[0:3]).reshape(-1))
        nom.t = (C.c_double * 3)(*(np.array(nom.t) + dx[12:15]))
        nom.v = (C.c_double * 3)(*(v + dx[6:9]))
        nom.b_g = (C.c_double * 3)(*(np.array(nom.b_g) + dx[3:6]))
        nom.b_a = (C.c_double * 3)(*(np.array(nom.b_a) + dx[9:12]))
        assert la.msckf_import_covariance(ha, _ffi.dptr(Pn), 0) == 0
        assert la.msckf_set_nominal(ha, C.byref(nom)) == 0
        return (time.perf_counter() - t0) * 1e6

    def path_b(dense):
        eng_b.propagate_imu(gyro, acc, dt)
        t0 = time.perf_counter()
        if dense:
            eng_b.run_rows(Hd, 0.01 * np.sqrt(np.diag(Rd)), Rd)
        else:
            eng_b.zero_velocity(sig_v)
        assert eng_b.commit_inject() == 0
        t1 = time.perf_counter()
        return (t1 - t0) * 1e6

    t = {"a": [], "b_zupt": [], "b_dense32": []}
    for i in range(warmup + reps):
        x = path_a(), path_b(False), path_b(True)
        if i >= warmup:
            for k, v in zip(t, x):
                t[k].append(v)
    out = {"N": N, "d": d, "reps": reps, "parent_lib": bool(parent_lib)}
    for k, v in t.items():
        out[f"{k}_us"] = float(np.median(v))
        out[f"{k}_p10_p90_us"] = [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
    # device time of one rows run (upload + two launches) per shape
    ev = Events(eng_b)
    out["device_us"] = {}
    for m, n_cols in ((3, 9), (3, 15), (6, d), (16, 15), (17, 15), (32, 15), (32, d)):
        H = rng.standard_normal((m, n_cols)) / s[None, :n_cols]
        Hp = np.zeros((m, d))
        Hp[:, :n_cols] = H
        P_now = eng_b.covariance()
        R = np.diag(np.einsum("ij,jk,ik->i", Hp, P_now, Hp) * rng.uniform(0.25, 4.0, m))
        r = 0.01 * np.sqrt(np.diag(R))
        dev = []
        for i in range(warmup + reps):
            eng_b.sync()
            ev.record(0)
            eng_b.run_rows(H, r, R)
            ev.record(1)
            us = ev.elapsed_us()
            if i >= warmup:
                dev.append(us)
        assert eng_b.result().status == 0
        out["device_us"][f"{m}x{n_cols}"] = float(np.median(dev))
    eng_a.close()
    eng_b.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clones", type=int, nargs="+", default=[30, 50])
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--parent-lib", default=None, help="a build of the library at the parent commit: path (a) runs on it")
    a = ap.parse_args()
    res = [bench(N, a.reps, a.warmup, a.parent_lib) for N in a.clones]
    for r in res:
        print(f"\nN = {r['N']} (d = {r['d']}), medians of {r['reps']} alternating rounds, host clock, us"
              f"{'' if r['parent_lib'] else '  [path (a) on the library under test]'}")
        print("| path | median | p10 - p90 |\n|---|---|---|")
        for k, label in (("a", "(a) get P + nominal, NumPy update + injection, import P + set nominal"),
                         ("b_zupt", "(b) zero_velocity + commit_inject"), ("b_dense32", "(b) run_rows 32 x d + commit_inject")):
            lo, hi = r[f"{k}_p10_p90_us"]
            print(f"| {label} | {r[f'{k}_us']:.0f} | {lo:.0f} - {hi:.0f} |")
        print("device time of a rows run (upload of H | r | R + two launches), HIP events, us: " +
              ", ".join(f"{k}: {v:.1f}" for k, v in r["device_us"].items()))
    print(json.dumps({"bench_rows": res}))


if __name__ == "__main__":
    main()
