#!/usr/bin/env python3
"""Generate `wide/edge_wide_tracks.npz`: one batch with tracks of more than 31 views through the REFERENCE's own
`MSCKF.update` (`MSCKF.py:570-614`; `np.linalg.qr` takes any track length, `:573-588`).

N = 40 clones, 24 tracks of 20 to 40 views, 30 % of them with one 400 px outlier view: 12 tracks hold more than 31 views
(the wide K1-K4 kernel, `csrc/k_feature_wide.h`), some of them are rejected by the gate and some accepted.  Like
`gen_match_golden.py` this imports `gen_golden` (the stub recipe of SURVEY.md Appendix A and `run_reference`), runs
only where the reference is mounted, and writes arrays and the versions triple only.  (The fixture sits in a directory of
its own: every `golden/*.npz` is read by the existing parity tests, whose engines hold 31 views.)

    python tests/golden/gen_wide_golden.py
"""
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden  # noqa: E402  (the stub modules and the reference on sys.path)
from msckf_amd import synth  # noqa: E402

NAME = "edge_wide_tracks"
SHAPE = dict(N=40, F=24, M=40, seed=24, variable_tracks=True, min_track=20, outlier_fraction=0.3)
WIDE_FROM = 32            # views from which a track is wide (MSCKF_MAX_TRACK + 1)
MIN_MARGIN = 1e-3         # no gate decision within this of its threshold: the fixture pins parity, not a borderline gate


def main():
    prob = synth.make_problem(**SHAPE)
    out = gen_golden.run_reference(prob)
    views = np.diff(prob.view_ptr)
    wide = views >= WIDE_FROM
    acc = out["accepted"].astype(bool)
    assert int(wide.sum()) >= 4 and (wide & acc).any() and (wide & ~acc).any(), (views.tolist(), acc.tolist())
    assert int(out["status"]) == 0 and float(out["min_gate_margin"]) >= MIN_MARGIN, float(out["min_gate_margin"])
    # P and P+ are 255 x 255 and random to the last bit: as full matrices they alone pass the size limit of a committed file.
    # Both are bit-symmetric (asserted), so their upper triangles are stored, row by row (np.triu_indices order).
    assert np.array_equal(prob.P, prob.P.T) and np.array_equal(out["P_new"], out["P_new"].T)
    iu = np.triu_indices(prob.d)
    arrays = dict(
        P_triu=prob.P[iu], cam_R=prob.cam_R, cam_t=prob.cam_t, cam_R0=prob.cam_R0, cam_t0=prob.cam_t0,
        gravity=prob.gravity, K=prob.K, sigma=np.float64(prob.sigma), view_ptr=prob.view_ptr,
        obs_uv=prob.obs_uv, obs_slot=prob.obs_slot, idp_base=prob.idp_base, idp_m=prob.idp_m, idp_rho=prob.idp_rho,
        status=out["status"], dx=out["dx"], P_new_triu=out["P_new"][iu], accepted=out["accepted"], gamma=out["gamma"],
        crit=out["crit"], n_rejected=out["n_rejected"], min_gate_margin=out["min_gate_margin"],
        versions=np.array([np.__version__, scipy.__version__, sys.version.split()[0]]))
    os.makedirs(os.path.join(HERE, "wide"), exist_ok=True)
    path = os.path.join(HERE, "wide", NAME + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{NAME}: accepted {int(acc.sum())} of {prob.F}, margin {float(out['min_gate_margin']):.2e}, {os.path.getsize(path) / 1024:.0f} KiB")
    print(f"{NAME}: {int(wide.sum())} wide tracks of {prob.F} ({int((wide & acc).sum())} accepted, {int((wide & ~acc).sum())} rejected), "
          f"views {int(views.min())}..{int(views.max())}")


if __name__ == "__main__":
    main()
