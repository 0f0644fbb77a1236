"""Host-side mirror of the reference's update interface.

`UpdateEngine.update_problem` is the flat call; `UpdateEngine.update` accepts
reference-shaped objects (an ordered `cameras` mapping, `Feature`-like records
with `keypoints`, `camera_indices`, `inverse_depth_point.{base,m,rho}`) exactly
like `MSCKF.update(features)` (reference `src/msckf/MSCKF.py:570`) reads them, and
then applies the state injection half of `MSCKF.correct` (`:616-661`) on the
host.  All arithmetic of the update itself runs in the HIP library.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _ffi
from .synth import SelectParams, TrackTable, UpdateProblem

_CHI2 = None


def chi2_table() -> np.ndarray:
    """chi2.ppf(0.95, dof) for dof = 0..512 (index 0 unused), generated once with
    scipy by tests/golden/gen_golden.py (reference `MSCKF.py:565-566`)."""
    global _CHI2
    if _CHI2 is None:
        _CHI2 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "chi2_ppf_095.npy"))
    return _CHI2


@dataclass
class UpdateResult:
    status: int              # 0 updated, 1 no-op (nothing accepted)
    dx: np.ndarray           # (d,)
    P_new: np.ndarray        # (d, d)
    accepted: np.ndarray     # (F,) uint8, input order
    stats: dict

    @property
    def n_rejected(self) -> int:
        """Features that went through the gate and failed it (unselected ones do not count)."""
        if "n_rejected" in self.stats:
            return int(self.stats["n_rejected"])
        return int(self.accepted.size - int(self.accepted.sum()))


@dataclass
class Selection:
    """Outcome of `get_valid_features` (reference `MSCKF.py:458-495`), input order."""
    flags: np.ndarray        # (F,) uint8: 1 valid, 2 lost, 4 inverse-depth point refreshed, 8 ... from the refined point
    idp_m: np.ndarray        # (F, 3) after the refresh
    idp_rho: np.ndarray      # (F,)
    world: np.ndarray        # (F, 3) triangulated points, NaN where none

    @property
    def valid(self) -> np.ndarray:
        return (self.flags & _ffi.SEL_VALID) > 0

    @property
    def lost(self) -> np.ndarray:
        return (self.flags & _ffi.SEL_LOST) > 0

    @property
    def refreshed(self) -> np.ndarray:
        return (self.flags & _ffi.SEL_REFRESHED) > 0

    @property
    def refined(self) -> np.ndarray:
        """Tracks whose point is the refined one (`SelectParams.refine_iters` > 0), a subset of `refreshed`."""
        return (self.flags & _ffi.SEL_REFINED) > 0


def exchange_split_rule(prob: UpdateProblem, shards, lib=None, handle=None) -> dict:
    """`UpdateEngine.exchange_split_rule` without an engine (the library's defaults; no GPU needed)."""
    lib = lib if lib is not None else _ffi.load()
    vp = np.ascontiguousarray(prob.view_ptr, dtype=np.int32)
    slots = np.ascontiguousarray(np.asarray(prob.obs_slot).reshape(-1), dtype=np.int32)
    bounds = np.ascontiguousarray([s[0] for s in shards] + [shards[-1][1]], dtype=np.int32)
    out = np.zeros(4, dtype=np.int32)
    flags = np.zeros((len(shards), int(prob.N)), dtype=np.uint8)
    rc = lib.msckf_exchange_split_rule(handle, int(prob.N), int(prob.F), _ffi.iptr(vp), _ffi.iptr(slots), len(shards),
                                       _ffi.iptr(bounds), _ffi.iptr(out), flags.ctypes.data)
    if rc != 0:
        raise _ffi.EngineError(rc, "msckf_exchange_split_rule")
    return {"split": bool(out[0]), "span": int(out[1]), "rows": int(out[2]), "total": int(out[3]), "flags": flags}


class UpdateEngine:
    """One context on one MI355X.  Not thread-safe (one engine per host thread)."""

    def __init__(self, max_clones: int = 30, max_features: int = 4096, max_track: int = 30,
                 device: int = 0, leaf_rows: int = 0, merge_arity: int = 0, plan: str = "auto", dtype: str = "f64",
                 wide_store: bool = False):
        """plan: "auto" = band pipeline (k_sweep) for tracks of up to 10 clone slots; longer ones are split into <= 10-slot
        blocks for that pipeline + a few remainder rows; "band" = no split: 90-column band tiles for tracks of
        11 - 15 slots, the merge tree beyond; "tree" = always the merge tree (A/B, tests).
        dtype: "f64" = the reference's arithmetic (parity 1e-8); "f32" = fp32 storage of the stacked system and
        the Joseph covariance update on the f32 matrix cores (BASELINE.json configs[4]; tolerance in DESIGN.md).
        wide_store: with `max_track` > 32 the engine has a track store (`tracks_*`, `load_tracks*`) only on request: rows of
        `max_track` views, which is also the batch limit (fp64 only; `MSCKF_FLAG_WIDE_STORE`).  Without it such an engine
        answers `ERR_ARG` to every store call; with `max_track` <= 32 it changes nothing."""
        # (up to MAX_TRACK: the batch limit; MAX_TRACK_ROW: rows of the track store only, a batch track holds MAX_TRACK; beyond: the
        #  batch limit, tracks of more than MAX_TRACK views on the wide K1-K4 kernel, and with wide_store the rows of the store)
        if max_track > _ffi.MAX_TRACK_WIDE:
            raise ValueError(f"max_track {max_track} > {_ffi.MAX_TRACK_WIDE}")
        if plan not in ("auto", "band", "tree"):
            raise ValueError("plan must be 'auto', 'band' or 'tree'")
        if dtype not in ("f64", "f32"):
            raise ValueError("dtype must be 'f64' or 'f32'")
        if wide_store and dtype == "f32" and max_track > _ffi.MAX_TRACK_ROW:
            raise ValueError(f"wide_store with dtype 'f32' and max_track {max_track} > {_ffi.MAX_TRACK_ROW}: the f32 stack takes "
                             f"tracks of {_ffi.MAX_TRACK} views, rows of more could never be loaded")
        self._lib = _ffi.load()               # (every argument check stands in front of the library)
        self.dtype = dtype
        cfg = _ffi.Config(_ffi.ABI_VERSION, device, max_clones, max_features, max_track, leaf_rows, merge_arity,
                          {"tree": _ffi.FLAG_TREE_PLAN, "band": _ffi.FLAG_BAND_ONLY}.get(plan, 0) | (_ffi.FLAG_WIDE_STORE if wide_store else 0),
                          _ffi.DTYPE_F32 if dtype == "f32" else _ffi.DTYPE_F64, 0)
        h = C.c_void_p()
        rc = self._lib.msckf_create(C.byref(h), C.byref(cfg))
        if rc != 0:
            raise _ffi.EngineError(rc, self._lib.msckf_strerror(rc).decode())
        self._h = h
        self.max_clones, self.max_features, self.max_track = max_clones, max_features, max_track
        self._N = 0
        self._F = 0
        self._rows_run = False                # the last run was run_rows / a fix: result() holds one verdict
        self._views = None      # views of the loaded batch where the caller's arrays told (set_view_sigma checks its length)
        self._desc_dim = 0      # D of the last tracks_match_frame that went in (track_descriptor trims to it)

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.msckf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, allow_noop=True):
        if rc == 0 or (allow_noop and rc == 1):
            return rc
        text = self._lib.msckf_strerror(rc).decode()
        if rc in (_ffi.ERR_HIP, _ffi.ERR_COMM):
            text += ": " + self._lib.msckf_last_error(self._h).decode()
        raise _ffi.EngineError(rc, text)

    # -- one-shot drop-in ---------------------------------------------------
    def update_problem(self, prob: UpdateProblem) -> UpdateResult:
        """Host arrays in, host arrays out: the arithmetic of `MSCKF.update` +
        the covariance update of `MSCKF.correct` (reference `MSCKF.py:570-614`)."""
        N, F, d = prob.N, prob.F, prob.d
        a = self._pack(prob)
        chi = _ffi.f64(chi2_table())
        dx = np.empty(d)                           # the library writes every entry of dx, P_out, accepted[:F]
        P_out = np.empty((d, d))
        acc = np.zeros(max(F, 1), dtype=np.uint8)
        st = _ffi.Stats()
        # (per-view noise: sigma_view behind idp_rho, or NULL -- msckf_update is this call with NULL)
        vs = None if prob.view_sigma is None else self._view_sigma(prob.view_sigma, int(a["view_ptr"][-1]))
        if prob.point_prior is not None:
            # (priors on the tracks' points behind sigma_view: msckf_update_prior; without them the call below, as ever)
            pc, keep = self._point_priors(prob.point_prior, F)
            rc = self._lib.msckf_update_prior(
                self._h, N, _ffi.dptr(a["P"]), _ffi.dptr(a["cam_R"]), _ffi.dptr(a["cam_t"]), _ffi.dptr(a["cam_R0"]),
                _ffi.dptr(a["cam_t0"]), _ffi.dptr(a["g"]), _ffi.dptr(a["Kinv"]), float(prob.sigma), F,
                _ffi.iptr(a["view_ptr"]), _ffi.dptr(a["obs_uv"]), _ffi.iptr(a["obs_slot"]), _ffi.dptr(a["idp_base"]),
                _ffi.dptr(a["idp_m"]), _ffi.dptr(a["idp_rho"]), None if vs is None else _ffi.dptr(vs), C.byref(pc), _ffi.dptr(chi),
                int(chi.size), _ffi.dptr(dx), _ffi.dptr(P_out), _ffi.uptr(acc), C.byref(st))
            del keep
            self._check(rc)
            self._N, self._F, self._views = N, F, int(a["view_ptr"][-1])
            return UpdateResult(rc, dx, P_out, acc[:F].copy(), st.as_dict())
        rc = self._lib.msckf_update_sigma(
            self._h, N, _ffi.dptr(a["P"]), _ffi.dptr(a["cam_R"]), _ffi.dptr(a["cam_t"]), _ffi.dptr(a["cam_R0"]),
            _ffi.dptr(a["cam_t0"]), _ffi.dptr(a["g"]), _ffi.dptr(a["Kinv"]), float(prob.sigma), F,
            _ffi.iptr(a["view_ptr"]), _ffi.dptr(a["obs_uv"]), _ffi.iptr(a["obs_slot"]), _ffi.dptr(a["idp_base"]),
            _ffi.dptr(a["idp_m"]), _ffi.dptr(a["idp_rho"]), None if vs is None else _ffi.dptr(vs), _ffi.dptr(chi), int(chi.size),
            _ffi.dptr(dx), _ffi.dptr(P_out), _ffi.uptr(acc), C.byref(st))
        self._check(rc)
        self._N, self._F, self._views = N, F, None if vs is None else int(vs.size)
        return UpdateResult(rc, dx, P_out, acc[:F].copy(), st.as_dict())

    _kinv_cache = (None, None)

    @classmethod
    def _kinv(cls, K) -> np.ndarray:
        """inv(K) as the reference forms it (`MSCKF.py:519`); the intrinsics rarely change between calls."""
        K = np.asarray(K, dtype=np.float64)
        key, val = cls._kinv_cache
        if key is None or key.shape != K.shape or not np.array_equal(key, K):
            val = _ffi.f64(np.linalg.inv(K))
            cls._kinv_cache = (K.copy(), val)
        return val

    @classmethod
    def _pack(cls, prob: UpdateProblem) -> dict:
        # (C-contiguous float64 / int32 arrays whatever their shape: the library takes addresses)
        return dict(
            P=_ffi.f64(prob.P), cam_R=_ffi.f64(prob.cam_R), cam_t=_ffi.f64(prob.cam_t),
            cam_R0=_ffi.f64(prob.cam_R0), cam_t0=_ffi.f64(prob.cam_t0),
            g=_ffi.f64(prob.gravity), Kinv=cls._kinv(prob.K),               # reference MSCKF.py:519
            view_ptr=_ffi.i32(prob.view_ptr), obs_uv=_ffi.f64(prob.obs_uv),
            obs_slot=_ffi.i32(prob.obs_slot), idp_base=_ffi.f64(prob.idp_base),
            idp_m=_ffi.f64(prob.idp_m), idp_rho=_ffi.f64(prob.idp_rho))

    # -- resident path ------------------------------------------------------
    def set_state(self, prob: UpdateProblem):
        a = self._pack(prob)
        chi = _ffi.f64(chi2_table())
        self._check(self._lib.msckf_set_state(
            self._h, prob.N, _ffi.dptr(a["P"]), _ffi.dptr(a["cam_R"]), _ffi.dptr(a["cam_t"]), _ffi.dptr(a["cam_R0"]),
            _ffi.dptr(a["cam_t0"]), _ffi.dptr(a["g"]), _ffi.dptr(a["Kinv"]), float(prob.sigma), _ffi.dptr(chi),
            int(chi.size)), allow_noop=False)
        if prob.N != self._N:                 # (another N drops the loaded batch; at the same N it stays, and so does its size)
            self._F = 0
        self._N = prob.N

    def set_features(self, prob: UpdateProblem):
        a = self._pack(prob)
        self._check(self._lib.msckf_set_features(
            self._h, prob.F, _ffi.iptr(a["view_ptr"]), _ffi.dptr(a["obs_uv"]), _ffi.iptr(a["obs_slot"]),
            _ffi.dptr(a["idp_base"]), _ffi.dptr(a["idp_m"]), _ffi.dptr(a["idp_rho"])), allow_noop=False)
        self._F = prob.F
        self._views = int(a["view_ptr"][-1])

    def load(self, prob: UpdateProblem):
        self.set_state(prob)
        self.set_features(prob)
        if prob.view_sigma is not None:
            self.set_view_sigma(prob.view_sigma)
        if prob.point_prior is not None:
            self.set_point_priors(prob.point_prior)

    @staticmethod
    def _point_priors(pri, F: int):
        """(msckf_point_priors, the arrays it points into) of a `synth.PointPriors` for a batch of F tracks."""
        if pri.F != F:
            raise ValueError(f"the priors name {pri.F} tracks, the batch holds {F}")
        has = np.ascontiguousarray(pri.has, dtype=np.uint8)
        mean, cov = _ffi.f64(pri.mean), _ffi.f64(pri.cov)
        pc = _ffi.PointPriorsC(_ffi.uptr(has), _ffi.dptr(mean), _ffi.dptr(cov), _ffi.PRIOR_AT_MEAN if pri.at_mean else 0, 0)
        return pc, (has, mean, cov)

    def set_point_priors(self, pri=None):
        """Priors on the points of the loaded batch's tracks (`msckf_set_point_priors`; not in the reference): a
        `synth.PointPriors` in the input order of the tracks -- p_j ~ N(mean[j], cov[j]) in the world frame where
        `has[j]`, three whitened rows in front of the null-space projection, 2M rows of the track in the update
        (a track of one view included); `at_mean` linearises a prior track at the mean.  `None` clears.  Call it
        after the batch load (`set_features`, `load_tracks`, `load_tracks_where`), before the run; the next batch
        load and `set_state` clear it.  `EngineError` (`ERR_ARG`) for a prior that is not finite, not bitwise
        symmetric or not positive definite, on a track of more than 30 views, or an f32 engine; (`ERR_STATE`)
        without a loaded batch or under a group exchange -- the priors in force stay as they were."""
        if pri is None:
            self._check(self._lib.msckf_set_point_priors(self._h, None), allow_noop=False)
            return
        pc, keep = self._point_priors(pri, self._F if self._F else pri.F)      # (no batch: the engine answers ERR_STATE, reading nothing)
        self._check(self._lib.msckf_set_point_priors(self._h, C.byref(pc)), allow_noop=False)
        del keep

    def prior_distance(self) -> np.ndarray:
        """(pbar - p_lin)^T Sigma_p^-1 (pbar - p_lin) per track of the last run at its linearisation point, 0 for a
        plain or skipped track (`msckf_get_prior_distance`; waits for the stream).  `EngineError` (`ERR_STATE`) when
        the loaded batch's last run had no priors or its results were voided since."""
        d2 = np.zeros(max(self._F, 1))
        self._check(self._lib.msckf_get_prior_distance(self._h, _ffi.dptr(d2)), allow_noop=False)
        return d2[:self._F].copy()

    @staticmethod
    def _view_sigma(view_sigma, n_views: int) -> np.ndarray:
        vs = _ffi.f64(np.asarray(view_sigma, dtype=np.float64).reshape(-1))
        if vs.size != n_views:
            raise ValueError(f"view_sigma holds {vs.size} entries, the batch {n_views} views")
        return vs

    def set_view_sigma(self, view_sigma=None):
        """Per-view measurement noise of the loaded batch (`msckf_set_view_sigma`): one standard deviation per view, in
        the input order of the views and in `sigma`'s units; `None` clears.  The next batch load or `set_state` clears
        them too.  Raises `ValueError` for a wrong length, `EngineError` (`ERR_ARG`) for an entry that is not finite or
        not > 0 and (`ERR_STATE`) without a loaded batch -- the weights in force stay as they were."""
        if view_sigma is None:
            self._check(self._lib.msckf_set_view_sigma(self._h, None), allow_noop=False)
            return
        vs = _ffi.f64(np.asarray(view_sigma, dtype=np.float64).reshape(-1))
        n = getattr(self, "_views", None)      # (views of the loaded batch; a batch of the track store: the caller counts them)
        if n is not None and vs.size != n:
            raise ValueError(f"view_sigma holds {vs.size} entries, the loaded batch {n} views")
        self._check(self._lib.msckf_set_view_sigma(self._h, _ffi.dptr(vs)), allow_noop=False)

    _ROBUST_LOSSES = {"huber": _ffi.ROBUST_HUBER, "cauchy": _ffi.ROBUST_CAUCHY}

    def set_robust(self, loss=None, k: float = 1.345, w_min: float = 0.05):
        """A robust loss on the reprojection residual in front of K1 (`msckf_set_robust`; not in the reference): every
        view is reweighted once at the linearisation point, `w_v = b_v max(sqrt(omega(s_v)), w_min)` with
        `s_v = b_v |e_v| / sigma` the whitened residual norm and `b_v` the base weight of `set_view_sigma` (else 1).
        `loss`: None (off), "huber" (`omega = min(1, k / s)`, typical k 1.345) or "cauchy" (`1 / (1 + (s / k)^2)`,
        typical k 2.385); a number is passed on as the C constant.  A setting of the engine: it survives `set_state`
        and batch loads, and every call that runs the update honours it, the one-shot and the reference-shaped ones
        included.  `EngineError` (`ERR_ARG`) for an unknown loss, k not finite or not > 0, w_min outside (0, 1]; the
        setting then stays as it was."""
        if loss is None:
            self._check(self._lib.msckf_set_robust(self._h, None), allow_noop=False)
            return
        if isinstance(loss, str):
            if loss not in self._ROBUST_LOSSES:
                raise ValueError("loss must be None, 'huber' or 'cauchy'")
            loss = self._ROBUST_LOSSES[loss]
        rp = _ffi.RobustParamsC(int(loss), 0, float(k), float(w_min))
        self._check(self._lib.msckf_set_robust(self._h, C.byref(rp)), allow_noop=False)

    def view_weights(self) -> dict:
        """`w` and `s` per view of the last run under `set_robust`, in the input order of the views, and `n_down`, the
        number of views whose factor `phi_v` was below 1 (`msckf_get_view_weights`; waits for the stream).  A track
        the run skipped reports `w = b`, `s = 0`.  `EngineError` (`ERR_STATE`) when the loaded batch's last run did not
        have the option on or its results were voided since."""
        n = getattr(self, "_views", None)
        # (a batch of the track store: the engine counts its views; w is finite for every view there is)
        cap = n if n is not None else max(self._F, 1) * self.max_track
        w, s = np.full(max(cap, 1), np.nan), np.full(max(cap, 1), np.nan)
        nd = np.zeros(1, dtype=np.int32)
        self._check(self._lib.msckf_get_view_weights(self._h, _ffi.dptr(w), _ffi.dptr(s), _ffi.iptr(nd)), allow_noop=False)
        if n is None:
            n = int(np.count_nonzero(~np.isnan(w)))
        return {"w": w[:n].copy(), "s": s[:n].copy(), "n_down": int(nd[0])}

    def run(self):
        self._check(self._lib.msckf_run(self._h), allow_noop=False)
        self._rows_run = False

    def run_compress(self):
        self._rows_run = False
        self._check(self._lib.msckf_run_compress(self._h), allow_noop=False)

    def sync(self):
        self._check(self._lib.msckf_sync(self._h), allow_noop=False)

    def run_timed(self, iters: int, stages: bool = False):
        """`iters` back-to-back device pipelines timed with HIP events on the
        engine's stream.  Returns (ms_total, [us_feature, us_qr, us_gain] or None)."""
        self._rows_run = False
        ms = C.c_float(0)
        st = (C.c_float * 3)()
        self._check(self._lib.msckf_run_timed(self._h, iters, C.byref(ms), st if stages else None), allow_noop=False)
        return float(ms.value), ([float(x) for x in st] if stages else None)

    def result(self) -> UpdateResult:
        d = 15 + 6 * self._N
        dx = np.zeros(d)
        P_out = np.zeros((d, d))
        acc = np.zeros(max(self._F, 1), dtype=np.uint8)
        st = _ffi.Stats()
        rc = self._check(self._lib.msckf_get_result(self._h, _ffi.dptr(dx), _ffi.dptr(P_out), _ffi.uptr(acc), C.byref(st)))
        n_acc = 1 if self._rows_run else self._F       # (a rows run: one verdict, whatever batch is loaded)
        return UpdateResult(rc, dx, P_out, acc[:n_acc].copy(), st.as_dict())

    def commit_covariance(self) -> int:
        return self._check(self._lib.msckf_commit_covariance(self._h))

    # -- f1: selection + triangulation in front of the update -----------------
    def set_tracks(self, tracks: TrackTable):
        """Lines and frame counters of the batch given to `set_features` (same order)."""
        b, dvec, c = _ffi.f64(tracks.line_base).reshape(-1), _ffi.f64(tracks.line_dir).reshape(-1), _ffi.f64(tracks.line_conf)
        lo, tr = _ffi.i32(tracks.lost_for), _ffi.i32(tracks.tracked_for)
        self._check(self._lib.msckf_set_tracks(self._h, _ffi.dptr(b), _ffi.dptr(dvec), _ffi.dptr(c), _ffi.iptr(lo),
                                               _ffi.iptr(tr)), allow_noop=False)

    def run_select(self, params: SelectParams, K):
        """Enqueue `get_valid_features` on the device; the following `run()` processes only
        the valid features, with their inverse-depth points refreshed in HBM.
        `params.refine_iters` in 1..32 adds the refinement of the triangulated points under the resident poses
        (at most that many Levenberg-Marquardt trials; `Selection.refined`, `select_refine_stats`); 0 is the
        reference's linear point; anything else raises `EngineError` (`ERR_ARG`)."""
        sp = _ffi.SelectParamsC()
        sp.min_frames_lost, sp.min_frames_tracked = int(params.min_frames_lost), int(params.min_frames_tracked)
        sp.use_parallax, sp.width, sp.height = int(bool(params.use_parallax)), int(params.width), int(params.height)
        sp.min_parallax_deg = float(params.min_parallax_deg)
        sp.refine_iters = int(params.refine_iters)
        sp.K = (C.c_double * 9)(*np.asarray(K, dtype=np.float64).reshape(9))
        self._check(self._lib.msckf_run_select(self._h, C.byref(sp)), allow_noop=False)

    def replan(self):
        """Plan the QR tree over the valid features only (syncs; optional after `run_select`)."""
        self._check(self._lib.msckf_replan(self._h), allow_noop=False)

    def clear_selection(self):
        self._check(self._lib.msckf_clear_selection(self._h), allow_noop=False)

    def selection(self) -> Selection:
        F = self._F
        fl = np.zeros(max(F, 1), dtype=np.uint8)
        m, rho, w = np.zeros((max(F, 1), 3)), np.zeros(max(F, 1)), np.zeros((max(F, 1), 3))
        self._check(self._lib.msckf_get_selection(self._h, _ffi.uptr(fl), _ffi.dptr(m), _ffi.dptr(rho), _ffi.dptr(w)),
                    allow_noop=False)
        return Selection(fl[:F].copy(), m[:F].copy(), rho[:F].copy(), w[:F].copy())

    def select_refine_stats(self) -> dict:
        """Per track of the last `run_select`, input order: `cost0` the weighted reprojection cost (normalised image
        coordinates, weights `line_conf`) at the linear point, `cost1` at the result (= `cost0` where the refined point
        was not kept), `trials`.  Zeros for tracks that were not attempted, and everywhere after a selection with
        `refine_iters` 0.  `EngineError` (`ERR_STATE`) without a selection."""
        F = self._F
        c0, c1, tr = np.zeros(max(F, 1)), np.zeros(max(F, 1)), np.zeros(max(F, 1), dtype=np.int32)
        self._check(self._lib.msckf_get_select_refine(self._h, _ffi.dptr(c0), _ffi.dptr(c1), _ffi.iptr(tr)), allow_noop=False)
        return {"cost0": c0[:F].copy(), "cost1": c1[:F].copy(), "trials": tr[:F].copy()}

    def time_select(self, iters: int = 50) -> float:
        """Average device microseconds of the selection (HIP events): the selection kernel and, with `refine_iters`
        > 0, the refinement launch behind it."""
        us = C.c_float(0)
        self._check(self._lib.msckf_debug_time_select(self._h, iters, C.byref(us)), allow_noop=False)
        return float(us.value)

    def select_problem(self, prob: UpdateProblem, tracks: TrackTable, params: SelectParams) -> Selection:
        """Flat `get_valid_features`: upload, select, download."""
        self.load(prob)
        self.set_tracks(tracks)
        self.run_select(params, prob.K)
        return self.selection()

    # -- f4: geometric consistency tests of the front end's matches ------------------
    def associate(self, matched_uv, R_cur, t_cur, K, epipolar_threshold: float = 5.0, homography_threshold: float = 5.0):
        """The per-(match, earlier view) tests of `add_camera_measurements` (reference `MSCKF.py:332-412`) for the
        loaded batch (the tracks BEFORE the new view) against one matched keypoint each (`matched_uv` (F, 2) pixels,
        NaN rows = no match).  Returns (result (F,) uint8: 0 kept, 1 epipolar failure, 2 homography failure,
        3 no match; fail_view (F,) int32)."""
        F = self._F
        ap = _ffi.AssocParamsC()
        ap.K = (C.c_double * 9)(*np.asarray(K, dtype=np.float64).reshape(9))
        ap.R_cur = (C.c_double * 9)(*np.asarray(R_cur, dtype=np.float64).reshape(9))
        ap.t_cur = (C.c_double * 3)(*np.asarray(t_cur, dtype=np.float64).reshape(3))
        ap.epipolar_threshold, ap.homography_threshold = float(epipolar_threshold), float(homography_threshold)
        uv = _ffi.f64(matched_uv).reshape(-1)
        if uv.size != 2 * F:
            raise ValueError("matched_uv must be (F, 2)")
        res = np.zeros(max(F, 1), dtype=np.uint8)
        fv = np.zeros(max(F, 1), dtype=np.int32)
        self._check(self._lib.msckf_run_associate(self._h, C.byref(ap), _ffi.dptr(uv), _ffi.uptr(res), _ffi.iptr(fv)),
                    allow_noop=False)
        return res[:F].copy(), fv[:F].copy()

    # -- f2 / f3: covariance resident in HBM between frames ---------------------
    def set_prior(self, P, gravity, K, sigma, cam_R=None, cam_t=None, cam_R0=None, cam_t0=None):
        """Upload the filter state once; N = 0 (the 15x15 IMU prior, no clone yet) is allowed."""
        P = _ffi.f64(P)
        N = (P.shape[0] - 15) // 6
        z9, z3 = np.zeros((0, 3, 3)), np.zeros((0, 3))
        cam_R = z9 if cam_R is None else cam_R
        cam_t = z3 if cam_t is None else cam_t
        prob = UpdateProblem(P=P, cam_R=np.asarray(cam_R, dtype=np.float64).reshape(N, 3, 3),
                             cam_t=np.asarray(cam_t, dtype=np.float64).reshape(N, 3),
                             cam_R0=np.asarray(cam_R if cam_R0 is None else cam_R0, dtype=np.float64).reshape(N, 3, 3),
                             cam_t0=np.asarray(cam_t if cam_t0 is None else cam_t0, dtype=np.float64).reshape(N, 3),
                             gravity=np.asarray(gravity, dtype=np.float64), K=np.asarray(K), sigma=float(sigma),
                             view_ptr=np.zeros(1, dtype=np.int32), obs_uv=np.zeros((0, 2)),
                             obs_slot=np.zeros(0, dtype=np.int32), idp_base=z3, idp_m=z3, idp_rho=np.zeros(0))
        self.set_state(prob)

    def propagate(self, Phi, Q):
        """Covariance half of `process_imu` (reference `MSCKF.py:236-244`); async."""
        a, b = _ffi.f64(Phi).reshape(-1), _ffi.f64(Q).reshape(-1)
        if a.size != 225 or b.size != 225:
            raise ValueError("Phi and Q are 15x15")
        self._check(self._lib.msckf_propagate(self._h, _ffi.dptr(a), _ffi.dptr(b)), allow_noop=False)

    def augment(self, J15, R, t):
        """`state_augmentation` (reference `MSCKF.py:250-265`): one more clone, P grows by 6."""
        j, r, tt = _ffi.f64(J15).reshape(-1), _ffi.f64(R).reshape(-1), _ffi.f64(t).reshape(-1)
        if j.size != 90 or r.size != 9 or tt.size != 3:
            raise ValueError("J15 is 6x15, R 3x3, t 3")
        self._check(self._lib.msckf_augment(self._h, _ffi.dptr(j), _ffi.dptr(r), _ffi.dptr(tt)), allow_noop=False)
        self._N += 1
        self._F = 0

    def remove_clones(self, slots):
        """Covariance half of `remove_cameras` (reference `MSCKF.py:751-757`)."""
        s = _ffi.i32(np.asarray(slots).reshape(-1))
        self._check(self._lib.msckf_remove_clones(self._h, int(s.size), _ffi.iptr(s)), allow_noop=False)
        self._N -= int(s.size)
        self._F = 0

    def set_poses(self, cam_R, cam_t, cam_R0=None, cam_t0=None):
        """Clone poses after the host's state injection (reference `MSCKF.py:642-661`)."""
        r, t = _ffi.f64(cam_R).reshape(-1), _ffi.f64(cam_t).reshape(-1)
        r0 = r if cam_R0 is None else _ffi.f64(cam_R0).reshape(-1)
        t0 = t if cam_t0 is None else _ffi.f64(cam_t0).reshape(-1)
        if r.size != 9 * self._N or t.size != 3 * self._N or r0.size != r.size or t0.size != t.size:
            raise ValueError("pose arrays do not match the number of clones")
        self._check(self._lib.msckf_set_poses(self._h, _ffi.dptr(r), _ffi.dptr(t), _ffi.dptr(r0), _ffi.dptr(t0)),
                    allow_noop=False)

    def covariance(self) -> np.ndarray:
        """The resident prior covariance (d x d)."""
        n = C.c_int32(0)
        self._check(self._lib.msckf_get_covariance(self._h, None, C.byref(n)), allow_noop=False)
        d = 15 + 6 * int(n.value)
        P = np.zeros((d, d))
        self._check(self._lib.msckf_get_covariance(self._h, _ffi.dptr(P), C.byref(n)), allow_noop=False)
        return P

    # -- the nominal state resident beside the covariance ----------------------
    def set_nominal(self, R, t, v, gravity, noise, T_W_I=None, T_W_C=None, b_g=None, b_a=None, R0=None, t0=None, v0=None,
                    planet_rate=None, T_I_C=None):
        """Upload the IMU state once (after `set_prior` / `set_state`): from here on `propagate_imu`, `augment_imu` and
        `commit_inject` keep it, the biases and the clone poses on the device.  `noise`: the 12x12 continuous noise
        covariance (reference `MSCKF.py:99-103`); `T_W_I`, `T_W_C`: (R, t) of the static IMU and camera frames, or
        `T_I_C` = (R, t) of their composition (`:252`).  Null state: `R0, t0, v0`, default the state itself."""
        from . import propagation
        if T_I_C is None:
            if T_W_I is None or T_W_C is None:
                raise ValueError("give T_I_C, or T_W_I and T_W_C")
            T_I_C = propagation.extrinsics(T_W_I, T_W_C)
        z3 = np.zeros(3)
        s = _ffi.NominalC()
        for name, val, size in (("R", R, 9), ("t", t, 3), ("v", v, 3), ("b_g", z3 if b_g is None else b_g, 3),
                                ("b_a", z3 if b_a is None else b_a, 3), ("R0", R if R0 is None else R0, 9),
                                ("t0", t if t0 is None else t0, 3), ("v0", v if v0 is None else v0, 3),
                                ("gravity", gravity, 3), ("planet_rate", z3 if planet_rate is None else planet_rate, 3),
                                ("Qc", noise, 144), ("T_I_C_R", T_I_C[0], 9), ("T_I_C_t", T_I_C[1], 3)):
            a = np.asarray(val, dtype=np.float64).reshape(-1)
            if a.size != size:
                raise ValueError(f"{name} has {a.size} entries, expected {size}")
            setattr(s, name, (C.c_double * size)(*a))
        self._check(self._lib.msckf_set_nominal(self._h, C.byref(s)), allow_noop=False)

    def nominal(self) -> dict:
        """The nominal state as it stands on the device (waits for the stream): `R, t, v, b_g, b_a, R0, t0, v0` of the
        IMU and `cam_R` (N, 3, 3), `cam_t` (N, 3) of the clones, whose null poses equal their poses."""
        s = _ffi.NominalC()
        N = self._N
        cam_R, cam_t = np.zeros((max(N, 1), 3, 3)), np.zeros((max(N, 1), 3))
        self._check(self._lib.msckf_get_nominal(self._h, C.byref(s), _ffi.dptr(cam_R), _ffi.dptr(cam_t)), allow_noop=False)
        out = {k: np.array(getattr(s, k)) for k in ("t", "v", "b_g", "b_a", "t0", "v0")}
        out["R"], out["R0"] = np.array(s.R).reshape(3, 3), np.array(s.R0).reshape(3, 3)
        out["cam_R"], out["cam_t"] = cam_R[:N], cam_t[:N]
        return out

    def propagate_imu(self, gyro, acc, dt):
        """`process_imu` (reference `MSCKF.py:160-248`) for up to `_ffi.IMU_BATCH_MAX` consecutive RAW samples in one
        call: integration, `Phi`, `Q` and the covariance on the device; async."""
        g, a, t = _ffi.f64(gyro).reshape(-1), _ffi.f64(acc).reshape(-1), _ffi.f64(dt).reshape(-1)
        if g.size != 3 * t.size or a.size != 3 * t.size:
            raise ValueError("gyro and acc are (n, 3), dt (n,)")
        self._check(self._lib.msckf_propagate_imu(self._h, int(t.size), _ffi.dptr(g), _ffi.dptr(a), _ffi.dptr(t)),
                    allow_noop=False)

    def augment_imu(self):
        """`state_augmentation` (reference `MSCKF.py:250-265`) from the resident IMU state; async."""
        self._check(self._lib.msckf_augment_imu(self._h), allow_noop=False)
        self._N += 1
        self._F = 0

    def commit_inject(self) -> int:
        """`commit_covariance` + the state injection of `MSCKF.correct` (reference `MSCKF.py:616-661`) on the device.
        A run is injected once: a second call for the same run raises `EngineError` (`ERR_STATE`) and changes nothing."""
        return self._check(self._lib.msckf_commit_inject(self._h))

    # -- direct measurement rows on the resident filter -------------------------
    @staticmethod
    def _rows_noise(R, m: int) -> np.ndarray:
        """`R` as an m x m matrix: a scalar sigma, a vector of m sigmas or the full matrix."""
        a = np.asarray(R, dtype=np.float64)
        if a.ndim == 0:
            return np.eye(m) * float(a) ** 2
        if a.ndim == 1:
            if a.size != m:
                raise ValueError(f"R holds {a.size} sigmas, the measurement {m} rows")
            return np.diag(a ** 2)
        return _ffi.f64(a)

    @staticmethod
    def _rows_crit(gate, m: int) -> float:
        """The critical value of `gate`: False / None not gated, True `chi2_table()[m]`, a float itself."""
        if gate is None or gate is False:
            return 0.0
        if gate is True:
            return float(chi2_table()[m])
        return float(gate)

    def run_rows(self, H, r, R, gate=False):
        """An update with the caller's rows `H` (m x n_cols, any n_cols <= d: the columns behind them are zero and are
        not padded), residual `r = z - h(nominal)` and noise `R` (scalar sigma, m sigmas or m x m) on the resident
        covariance; async.  The result is read by `result`, kept by `commit_covariance` / `commit_inject`.
        `gate`: True gates at `chi2_table()[m]`, a float at that value."""
        H = _ffi.f64(np.atleast_2d(np.asarray(H, dtype=np.float64)))
        r = _ffi.f64(r).reshape(-1)
        m, n_cols = (int(H.shape[0]), int(H.shape[1])) if H.size else (0, 0)
        if r.size != m:
            raise ValueError(f"r holds {r.size} entries, H {m} rows")
        Rm = self._rows_noise(R, m)
        if Rm.shape != (m, m):
            raise ValueError(f"R is {Rm.shape}, expected ({m}, {m})")
        self._check(self._lib.msckf_run_rows(self._h, m, n_cols, _ffi.dptr(H), _ffi.dptr(r), _ffi.dptr(Rm),
                                             self._rows_crit(gate, m)), allow_noop=False)
        self._rows_run = True

    def update_rows(self, H, r, R, gate=False) -> UpdateResult:
        """`run_rows` + `result`."""
        self.run_rows(H, r, R, gate)
        return self.result()

    def _run_fix(self, which: int, z, R, gate):
        z = _ffi.f64(z).reshape(-1)
        if z.size != 3:
            raise ValueError("z has 3 entries")
        Rm = self._rows_noise(R, 3)
        if Rm.shape != (3, 3):
            raise ValueError(f"R is {Rm.shape}, expected (3, 3)")
        self._check(self._lib.msckf_run_fix(self._h, which, _ffi.dptr(z), _ffi.dptr(Rm), self._rows_crit(gate, 3)),
                    allow_noop=False)
        self._rows_run = True

    def velocity_fix(self, z, R, gate=False):
        """A velocity measurement `z` (world frame) against the resident nominal state: the device forms `r = z - v`
        behind whatever `propagate_imu` left pending, no read-back; async."""
        self._run_fix(_ffi.FIX_VELOCITY, z, R, gate)

    def position_fix(self, z, R, gate=False):
        """A position measurement `z` of the IMU in the world frame: `r = z - t_WI` formed on the device; async."""
        self._run_fix(_ffi.FIX_POSITION, z, R, gate)

    def zero_velocity(self, sigma, gate=False):
        """A zero-velocity update at standstill: `velocity_fix` with z = 0."""
        self._run_fix(_ffi.FIX_VELOCITY, np.zeros(3), sigma, gate)

    def rows_gate(self):
        """(gamma, applied) of the last rows run; waits for it."""
        g = np.zeros(1)
        a = np.zeros(1, dtype=np.int32)
        self._check(self._lib.msckf_get_rows_gate(self._h, _ffi.dptr(g), _ffi.iptr(a)), allow_noop=False)
        return float(g[0]), bool(a[0])

    # -- the track store: views and bases resident, batches by track id --------
    def tracks_reset(self):
        """Empty the track store."""
        self._check(self._lib.msckf_tracks_reset(self._h), allow_noop=False)

    def tracks_observe(self, ids, uv, score):
        """One view of the newest clone for each listed track (reference `MSCKF.py:403-411`, `:420-434`): `uv` (n, 2)
        pixels, `score` (n,).  Unknown ids create tracks.  Direction, line and inverse-depth point are formed on the
        device from the resident pose; async."""
        i, u, s = _ffi.i32(np.asarray(ids).reshape(-1)), _ffi.f64(uv).reshape(-1), _ffi.f64(score).reshape(-1)
        if u.size != 2 * i.size or s.size != i.size:
            raise ValueError("uv is (n, 2), score (n,)")
        self._check(self._lib.msckf_tracks_observe(self._h, int(i.size), _ffi.iptr(i), _ffi.dptr(u), _ffi.dptr(s)),
                    allow_noop=False)

    def tracks_remove(self, ids):
        """Delete tracks (reference `MSCKF.py:739-741`)."""
        i = _ffi.i32(np.asarray(ids).reshape(-1))
        self._check(self._lib.msckf_tracks_remove(self._h, int(i.size), _ffi.iptr(i)), allow_noop=False)

    def load_tracks(self, ids, lost_for, tracked_for):
        """`set_features` + `set_tracks` for the listed tracks of the store, in the listed order; their bases are the
        resident clone positions.  `lost_for`, `tracked_for`: the front end's counters."""
        i = _ffi.i32(np.asarray(ids).reshape(-1))
        lo, tr = _ffi.i32(np.asarray(lost_for).reshape(-1)), _ffi.i32(np.asarray(tracked_for).reshape(-1))
        if lo.size != i.size or tr.size != i.size:
            raise ValueError("lost_for and tracked_for are (F,)")
        self._check(self._lib.msckf_tracks_load(self._h, int(i.size), _ffi.iptr(i), _ffi.iptr(lo), _ffi.iptr(tr)),
                    allow_noop=False)
        self._F = int(i.size)
        self._views = None

    def tracks_frame(self, ids, uv, score, K, epipolar_threshold: float = 5.0, homography_threshold: float = 5.0):
        """A frame's matches on the store (reference `MSCKF.py:332-438`): each (track id, keypoint, score) is tested against
        every stored view of its track with the resident poses; those that pass are appended as `tracks_observe` would,
        unknown ids create tracks, and the stored `lost_for` / `tracked_for` counters follow (unlisted tracks: lost + 1).
        Returns (result (n,) uint8: 0 appended, 1 epipolar failure, 2 homography failure, 4 created; fail_view (n,)
        int32).  Blocking."""
        i, u, s = _ffi.i32(np.asarray(ids).reshape(-1)), _ffi.f64(uv).reshape(-1), _ffi.f64(score).reshape(-1)
        if u.size != 2 * i.size or s.size != i.size:
            raise ValueError("uv is (n, 2), score (n,)")
        fp = _ffi.FrameParamsC()
        fp.K = (C.c_double * 9)(*np.asarray(K, dtype=np.float64).reshape(9))
        fp.epipolar_threshold, fp.homography_threshold = float(epipolar_threshold), float(homography_threshold)
        n = int(i.size)
        res, fv = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
        self._check(self._lib.msckf_tracks_frame(self._h, C.byref(fp), n, _ffi.iptr(i), _ffi.dptr(u), _ffi.dptr(s),
                                                 _ffi.uptr(res), _ffi.iptr(fv)), allow_noop=False)
        return res[:n].copy(), fv[:n].copy()

    # -- frame intake from descriptors: the match runs on the device against the store's rows --------
    @staticmethod
    def _desc(descriptors):
        """(n, D) descriptors as fp32 (XFeat's dtype): fp64 input, such as the data set's CSV descriptors, is rounded here."""
        d = _ffi.f32(descriptors)
        if d.ndim != 2:
            raise ValueError("descriptors are (n, D)")
        return d

    def set_match_options(self, search_radius=None, min_margin=None):
        """The match's two defences against repeated texture (`msckf_tracks_set_match_options`; not in the reference, off
        by default).  `search_radius` (pixels; None or 0: off; `inf` is legal): a track only meets the keypoints within
        that distance of its last stored keypoint.  `min_margin` (None or 0: off): a pair also needs its similarity to
        beat the second best of its row and of its column by more than the margin.  The rule in full stands in
        `include/msckf_mi355x.h`.  A setting of the engine: `tracks_reset` and `set_state` leave it alone.
        `EngineError` (`ERR_ARG`) for a negative or NaN value; the setting then stays as it was."""
        if search_radius is None and min_margin is None:
            self._check(self._lib.msckf_tracks_set_match_options(self._h, None), allow_noop=False)
            return
        mo = _ffi.MatchOptionsC(float(search_radius or 0.0), float(min_margin or 0.0))
        self._check(self._lib.msckf_tracks_set_match_options(self._h, C.byref(mo)), allow_noop=False)

    def tracks_match(self, descriptors, min_cosine_similarity: float = 0.82, keypoints=None):
        """The mutual-nearest-neighbour match of a frame's descriptors against the store's rows (reference
        `FeatureExtractor.match`, `FeatureExtractor.py:62-84`); the store is untouched.  With `keypoints` (n, 2) the
        match runs under the search window of `set_match_options` (`msckf_tracks_match_at`); without them it raises
        `EngineError` (`ERR_STATE`) while a radius is set.  Returns (track id (n,) int32, -1 where unmatched; similarity
        (n,) fp32, 0 where unmatched).  Blocking."""
        d = self._desc(descriptors)
        n, D = d.shape
        ids, sim = np.full(max(n, 1), -1, dtype=np.int32), np.zeros(max(n, 1), dtype=np.float32)
        if keypoints is None:
            rc = self._lib.msckf_tracks_match(self._h, float(min_cosine_similarity), int(D), int(n), _ffi.dptr(d),
                                              _ffi.iptr(ids), _ffi.dptr(sim))
        else:
            u = _ffi.f64(keypoints).reshape(-1)
            if u.size != 2 * n:
                raise ValueError("keypoints are (n, 2)")
            rc = self._lib.msckf_tracks_match_at(self._h, float(min_cosine_similarity), int(D), int(n), _ffi.dptr(d),
                                                 _ffi.dptr(u), _ffi.iptr(ids), _ffi.dptr(sim))
        self._check(rc, allow_noop=False)
        return ids[:n].copy(), sim[:n].copy()

    def tracks_match_report(self):
        """The table of the last match, in the order the tracks were created: (track id (T,) int32, reason code (T,)
        uint8: 0 paired, 1 no keypoint inside the window, 2 not mutual, 3 below the threshold, 4 below the margin).
        Empty after `tracks_reset` / `set_state`.  Blocking."""
        T = C.c_int32(0)
        self._check(self._lib.msckf_tracks_match_report(self._h, C.addressof(T), None, None, 0), allow_noop=False)
        cap = max(int(T.value), 1)
        ids, why = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint8)
        self._check(self._lib.msckf_tracks_match_report(self._h, C.addressof(T), _ffi.iptr(ids), _ffi.uptr(why), cap),
                    allow_noop=False)
        return ids[:int(T.value)].copy(), why[:int(T.value)].copy()

    def tracks_match_frame(self, keypoints, descriptors, scores, K, first_new_id: int, min_cosine_similarity: float = 0.82,
                           epipolar_threshold: float = 5.0, homography_threshold: float = 5.0):
        """A frame as (keypoints (n, 2), descriptors (n, D), scores (n,)) on the store: the else-branch of the reference's
        `add_camera_measurements` (`MSCKF.py:315-444`).  Matched pairs go through `tracks_frame`'s tests, every unmatched
        keypoint creates a track with ids `first_new_id, +1, ...` in ascending keypoint order, the counters follow and all
        match rows are recomputed.  Returns None when the reference skips the frame (no keypoint, `:286`; no pair matched,
        `:320`: nothing changed), else (ids (n,) int32, result (n,) uint8: 0 appended, 1 / 2 epipolar / homography failure,
        4 created; fail_view (n,) int32; similarity (n,) fp32).  Blocking."""
        d = self._desc(descriptors)
        n, D = d.shape
        u, s = _ffi.f64(keypoints).reshape(-1), _ffi.f64(scores).reshape(-1)
        if u.size != 2 * n or s.size != n:
            raise ValueError("keypoints are (n, 2), scores (n,)")
        mp = _ffi.MatchParamsC()
        mp.K = (C.c_double * 9)(*np.asarray(K, dtype=np.float64).reshape(9))
        mp.epipolar_threshold, mp.homography_threshold = float(epipolar_threshold), float(homography_threshold)
        mp.min_cosine_similarity, mp.desc_dim, mp.first_new_id = float(min_cosine_similarity), int(D), int(first_new_id)
        ids, fv = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        res, sim = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.float32)
        rc = self._check(self._lib.msckf_tracks_match_frame(self._h, C.byref(mp), int(n), _ffi.dptr(d), _ffi.dptr(u), _ffi.dptr(s),
                                                            _ffi.iptr(ids), _ffi.uptr(res), _ffi.iptr(fv), _ffi.dptr(sim)))
        if rc == _ffi.NOOP:
            return None
        self._desc_dim = int(D)
        return ids[:n].copy(), res[:n].copy(), fv[:n].copy(), sim[:n].copy()

    def frame_from_extracted(self, keypoints, descriptors, scores, K, first_new_id: int, **kw):
        """`tracks_match_frame` behind the reference's score floor (`MSCKF.py:281-284`): keypoints whose score is below
        half the frame's mean score (`np.mean`) are dropped first.  Returns (kept, out): the indices of the keypoints that
        went in and what `tracks_match_frame` returned for them (None: the frame was skipped)."""
        scores = np.asarray(scores)
        kept = np.nonzero(scores >= 0.5 * np.mean(scores))[0] if scores.size else np.zeros(0, dtype=np.int64)
        d = np.asarray(descriptors)
        d = d[kept] if d.ndim == 2 else d.reshape(0, 1)
        return kept, self.tracks_match_frame(np.asarray(keypoints).reshape(-1, 2)[kept], d, scores[kept], K, first_new_id, **kw)

    def track_descriptor(self, track_id: int):
        """(match row (D,), per-view descriptors (M, D)) of one track as they stand on the device, fp32.  Blocking."""
        row = np.zeros(_ffi.DESC_DIM, dtype=np.float32)
        views = np.zeros(max(self.max_track, _ffi.MAX_TRACK_ROW) * _ffi.DESC_DIM, dtype=np.float32)
        M = C.c_int32(0)
        self._check(self._lib.msckf_tracks_descriptor(self._h, int(track_id), _ffi.dptr(row), C.addressof(M), _ffi.dptr(views)),
                    allow_noop=False)
        D = self._desc_dim
        return row[:D].copy(), views[:int(M.value) * D].reshape(int(M.value), D).copy()

    def load_tracks_where(self, slots=None) -> np.ndarray:
        """`load_tracks` with the stored counters for every track (`slots` None or empty: `process_features`' candidates)
        or every track with a view in one of the listed clone slots (the prune paths), in the order the tracks were
        created.  Returns their ids: the input order of `accepted`, `flags` and `selection()`."""
        sl = _ffi.i32(np.zeros(0) if slots is None else np.asarray(slots).reshape(-1))
        cap = max(self.tracks_count()[0], 1)
        ids, F = np.zeros(cap, dtype=np.int32), C.c_int32(0)
        self._check(self._lib.msckf_tracks_load_where(self._h, int(sl.size), _ffi.iptr(sl), C.addressof(F), _ffi.iptr(ids), cap),
                    allow_noop=False)
        self._F = int(F.value)
        self._views = None
        return ids[:self._F].copy()

    def tracks_counters(self, ids):
        """(lost_for, tracked_for) of the listed tracks as the store keeps them."""
        i = _ffi.i32(np.asarray(ids).reshape(-1))
        lo, tr = np.zeros(max(i.size, 1), dtype=np.int32), np.zeros(max(i.size, 1), dtype=np.int32)
        self._check(self._lib.msckf_tracks_counters(self._h, int(i.size), _ffi.iptr(i), _ffi.iptr(lo), _ffi.iptr(tr)),
                    allow_noop=False)
        return lo[:i.size].copy(), tr[:i.size].copy()

    def tracks_clone_views(self) -> np.ndarray:
        """Views per clone slot (`number_of_features_per_camera`, reference `MSCKF.py:712-716`); zero: a clone without features."""
        out = np.zeros(max(self._N, 1), dtype=np.int32)
        self._check(self._lib.msckf_tracks_clone_views(self._h, _ffi.iptr(out)), allow_noop=False)
        return out[:self._N].copy()

    def track(self, track_id: int) -> dict:
        """One track as it stands on the device (waits for the stream): `slots, uv, dir, conf, line_base, idp_base,
        idp_m, idp_rho, anchor_slot` (-1 once the anchor clone was removed: the base is frozen)."""
        V = max(self.max_track, _ffi.MAX_TRACK_ROW)
        M, anchor = C.c_int32(0), C.c_int32(0)
        rho = C.c_double(0)
        slots = np.zeros(V, dtype=np.int32)
        uv, d, conf, lb = np.zeros((V, 2)), np.zeros((V, 3)), np.zeros(V), np.zeros((V, 3))
        ib, m = np.zeros(3), np.zeros(3)
        self._check(self._lib.msckf_tracks_get(
            self._h, int(track_id), C.addressof(M), _ffi.iptr(slots), _ffi.dptr(uv), _ffi.dptr(d), _ffi.dptr(conf),
            _ffi.dptr(lb), _ffi.dptr(ib), _ffi.dptr(m), C.addressof(rho), C.addressof(anchor)), allow_noop=False)
        n = int(M.value)
        return dict(slots=slots[:n].copy(), uv=uv[:n].copy(), dir=d[:n].copy(), conf=conf[:n].copy(),
                    line_base=lb[:n].copy(), idp_base=ib, idp_m=m, idp_rho=float(rho.value), anchor_slot=int(anchor.value))

    def tracks_count(self):
        """(tracks, views) the store holds."""
        nt, nv = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.msckf_tracks_count(self._h, C.addressof(nt), C.addressof(nv)), allow_noop=False)
        return int(nt.value), int(nv.value)

    def tracks_dropped(self) -> np.ndarray:
        """Ids of the tracks the last `remove_clones` deleted (left without a view)."""
        n = self._lib.msckf_tracks_dropped(self._h, None, 0)
        if n < 0:
            self._check(n, allow_noop=False)
        out = np.zeros(max(n, 1), dtype=np.int32)
        self._lib.msckf_tracks_dropped(self._h, _ffi.iptr(out), int(n))
        return out[:n].copy()

    @property
    def n_clones(self) -> int:
        return self._N

    # -- sharded path -------------------------------------------------------
    def block_doubles(self) -> int:
        return int(self._lib.msckf_block_doubles(self._h))

    def export_block(self, dst_ptr: Optional[int] = None):
        """Copy the local compressed block [R | Q^T r].  With `dst_ptr` (a device
        address) the copy stays in HBM; otherwise a host array is returned."""
        n_acc = C.c_int32(0)
        if dst_ptr is not None:
            self._check(self._lib.msckf_export_block(self._h, C.c_void_p(dst_ptr), 1, C.byref(n_acc)), allow_noop=False)
            return None, int(n_acc.value)
        dc = 6 * self._N
        blk = np.zeros((dc, dc + 1))
        self._check(self._lib.msckf_export_block(self._h, blk.ctypes.data_as(C.c_void_p), 0, C.byref(n_acc)),
                    allow_noop=False)
        return blk, int(n_acc.value)

    def merge_gain(self, blocks, total_accepted: int, n_blocks: Optional[int] = None):
        """Root side: QR-merge the gathered blocks and run K6-K7.  `blocks` is a
        host array (G, 6N, 6N+1) or an int device address (then pass n_blocks)."""
        self._rows_run = False
        if isinstance(blocks, (int, np.integer)):
            self._check(self._lib.msckf_run_merge_gain(self._h, C.c_void_p(int(blocks)), int(n_blocks), 1,
                                                       int(total_accepted)), allow_noop=False)
        else:
            b = _ffi.f64(blocks)
            self._check(self._lib.msckf_run_merge_gain(self._h, b.ctypes.data_as(C.c_void_p), int(b.shape[0]), 0,
                                                       int(total_accepted)), allow_noop=False)

    # -- group exchange: the sharded band pipeline ------------------------------
    @staticmethod
    def max_span(prob: UpdateProblem) -> int:
        """Longest track of the batch in clone slots (last slot - first slot + 1)."""
        if prob.F == 0:
            return 0
        vp = np.asarray(prob.view_ptr)
        slots = np.asarray(prob.obs_slot).reshape(-1)
        lo = np.minimum.reduceat(slots, vp[:-1])
        hi = np.maximum.reduceat(slots, vp[:-1])
        return int((hi - lo + 1).max())

    def band_ok(self, prob: UpdateProblem) -> bool:
        """True when every shard of `prob` is planned as the band pipeline ON THIS ENGINE: the library's own
        rule (`msckf_band_rule`: plan flag, sweep tile width, LDS budget), asked with the whole batch's longest
        track, so that all ranks agree before sharding.  Then the ranks may exchange group triangles
        (`export_groups` / `merge_groups`); otherwise root blocks (`export_block` / `merge_gain`)."""
        if prob.F == 0:
            return False
        rc = self._lib.msckf_band_rule(self._h, int(prob.N), self.max_span(prob))
        if rc < 0:
            self._check(rc, allow_noop=False)
        return rc >= 1

    def set_group_exchange(self, on: bool = True):
        """Plan the following batches with the group-record layout (call before `load`)."""
        self._check(self._lib.msckf_set_group_exchange(self._h, 1 if on else 0), allow_noop=False)

    def set_exchange_span(self, max_span: int):
        """Tell the engine the longest track of the WHOLE batch (clone slots) before its shard is loaded: every rank
        then lays its group record out for the sweep mode of the whole batch (also the ring-buffered modes, N > 37
        or tracks of 11 - 15 slots).  0 = not told (60-column k_sweep form only)."""
        self._check(self._lib.msckf_set_exchange_span(self._h, int(max_span)), allow_noop=False)

    def exchange_split_rule(self, prob: UpdateProblem, shards) -> dict:
        """Split records for the WHOLE batch `prob` cut into `shards` ([lo, hi) per rank) -- the same answer on every rank
        (`msckf_exchange_split_rule`): `split`, the band `span` after the split (for `set_exchange_span`), the remainder
        `rows` one record holds and their `total` bound (for `set_exchange_split`), the (world, N) uint8 group `flags` of
        every shard's record (for `merge_groups_flags`)."""
        return exchange_split_rule(prob, shards, self._lib, self._h)

    def set_exchange_split(self, rows: int, total: int = 0):
        """Record capacity for split records (the rule's `rows` / `total`; 0 = off: long tracks keep root blocks).  Same value
        on every rank, before `load`."""
        self._check(self._lib.msckf_set_exchange_split(self._h, int(rows), int(total)), allow_noop=False)

    def group_record_doubles(self) -> int:
        return int(self._lib.msckf_group_record_doubles(self._h))

    def export_groups(self, dst_ptr: Optional[int] = None, count: bool = True):
        """The shard's group triangles (one record, accepted count included) after `run_compress`; host array
        or HBM address.  `count=False` skips reading the gate results back (returns -1 for the count)."""
        n_acc = C.c_int32(-1)
        if dst_ptr is not None:
            self._check(self._lib.msckf_export_groups(self._h, C.c_void_p(dst_ptr), 1, C.byref(n_acc) if count else None),
                        allow_noop=False)
            return None, int(n_acc.value)
        rec = np.zeros(self.group_record_doubles())
        self._check(self._lib.msckf_export_groups(self._h, rec.ctypes.data_as(C.c_void_p), 0, C.byref(n_acc)),
                    allow_noop=False)
        return rec, int(n_acc.value)

    def merge_groups(self, records, total_accepted: int = -1, n_records: Optional[int] = None):
        """Root side: fold the shards' group triangles, one root sweep, K6-K7.  `records` is a host array
        (G, record_doubles) or an int device address (then pass n_records); `total_accepted` < 0 takes the
        sum of the counts the shards wrote into their records."""
        self._rows_run = False
        if isinstance(records, (int, np.integer)):
            self._check(self._lib.msckf_run_merge_groups(self._h, C.c_void_p(int(records)), int(n_records), 1,
                                                         int(total_accepted)), allow_noop=False)
        else:
            b = _ffi.f64(records)
            self._check(self._lib.msckf_run_merge_groups(self._h, b.ctypes.data_as(C.c_void_p), int(b.shape[0]), 0,
                                                         int(total_accepted)), allow_noop=False)

    def merge_groups_flags(self, records_ptr: int, n_records: int, flags: np.ndarray):
        """`merge_groups` without any device-to-host traffic: `flags` (n_records, N) uint8 says which first-slot
        groups each shard's record carries (the caller partitioned the batch, so it knows); the accepted counts
        are summed on the device.  `records_ptr` is an HBM address."""
        self._rows_run = False
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        self._check(self._lib.msckf_run_merge_groups_flags(self._h, C.c_void_p(int(records_ptr)), int(n_records), 1,
                                                           fl.ctypes.data), allow_noop=False)

    # -- RCCL exchange behind the C-ABI (no PyTorch) -----------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(_ffi.COMM_ID_BYTES)
        self._check(self._lib.msckf_comm_unique_id(buf), allow_noop=False)
        return buf.raw

    def comm_init(self, rank: int, world: int, uid: bytes):
        if len(uid) != _ffi.COMM_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        self._check(self._lib.msckf_comm_init(self._h, int(rank), int(world), C.c_char_p(uid)), allow_noop=False)

    def comm_destroy(self):
        self._check(self._lib.msckf_comm_destroy(self._h), allow_noop=False)

    def comm_buffer(self, n_doubles: int) -> int:
        """HBM scratch of the engine (address), e.g. the receive side of the gather on the merging rank."""
        p = self._lib.msckf_comm_buffer(self._h, int(n_doubles) * 8)
        if not p:
            raise _ffi.EngineError(_ffi.ERR_HIP, "comm buffer allocation failed")
        return int(p)

    def comm_gather(self, send_ptr: int, recv_ptr: int, count: int, root: int = 0):
        self._check(self._lib.msckf_comm_gather(self._h, C.c_void_p(int(send_ptr)), C.c_void_p(int(recv_ptr) if recv_ptr else None),
                                                int(count), int(root)), allow_noop=False)

    def comm_broadcast(self, ptr: int, count: int, root: int = 0):
        self._check(self._lib.msckf_comm_broadcast(self._h, C.c_void_p(int(ptr)), int(count), int(root)), allow_noop=False)

    def comm_allreduce(self, ptr: int, count: int, op: str = "sum"):
        self._check(self._lib.msckf_comm_allreduce(self._h, C.c_void_p(int(ptr)), int(count), 1 if op == "max" else 0),
                    allow_noop=False)

    def comm_put(self, dst_ptr: int, host: np.ndarray):
        a = _ffi.f64(host)
        self._check(self._lib.msckf_comm_put(self._h, C.c_void_p(int(dst_ptr)), a.ctypes.data, a.nbytes), allow_noop=False)

    def comm_get(self, src_ptr: int, n_doubles: int) -> np.ndarray:
        out = np.empty(int(n_doubles))
        self._check(self._lib.msckf_comm_get(self._h, out.ctypes.data, C.c_void_p(int(src_ptr)), out.nbytes), allow_noop=False)
        return out

    def result_host(self):
        """dx, P+ of the result range as host arrays without the gate bookkeeping (two copies: dx and P_out each
        from its own address)."""
        d = 15 + 6 * self._N
        dx = self.comm_get(self.device_pointer(0), d)
        P = self.comm_get(self.device_pointer(1), d * d)
        return dx, P.reshape(d, d)

    def device_pointer(self, which: int) -> int:
        """0 dx (dx | P_out contiguous for the current N), 1 P_out, 2 root block, 3 group record of the shard,
        4 prior covariance, 5 result range (status | dx | P_out | gate bytes), 6 its gate bytes."""
        return int(self._lib.msckf_device_pointer(self._h, int(which)))

    # -- sharded update: gate results riding with the exchange ---------------------------------
    def set_exchange_mask(self, bounds=None):
        """`bounds` (n_shards + 1,): shard r holds features [bounds[r], bounds[r+1]) of the whole batch; None
        switches the ride-along off.  Call before `load` / `set_features` (the record layout changes)."""
        if bounds is None:
            self._check(self._lib.msckf_set_exchange_mask(self._h, 0, None), allow_noop=False)
            self._F_total = 0
            return
        b = _ffi.i32(np.asarray(bounds).reshape(-1))
        self._check(self._lib.msckf_set_exchange_mask(self._h, int(b.size) - 1, _ffi.iptr(b)), allow_noop=False)
        self._F_total = int(b[-1])

    def gate_bytes(self) -> np.ndarray:
        """Gate byte per feature of the loaded batch, input order, as the group records carry them: 1 accepted, 0 rejected
        by the chi-square test, 2 gate matrix not SPD, 3 not selected (the root-block fallback exchange ships them, so
        that `shared_result` counts `n_rejected` and `not_spd` as every other path does)."""
        return self.gate_codes()[0]

    def gate_codes(self):
        """(codes (F,) uint8 in input order, block_codes, block_track): the gate's verdict per track and, for the narrow
        and remainder blocks of split long tracks, the byte each inherited and the input index of its track."""
        F = self._F
        nb = C.c_int32(0)
        codes = np.zeros(max(F, 1), dtype=np.uint8)
        self._check(self._lib.msckf_debug_gate_codes(self._h, _ffi.uptr(codes), C.addressof(nb), None, None), allow_noop=False)
        n = int(nb.value)
        bc, bt = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
        if n:
            self._check(self._lib.msckf_debug_gate_codes(self._h, None, None, _ffi.uptr(bc), _ffi.iptr(bt)), allow_noop=False)
        return codes[:F].copy(), bc[:n].copy(), bt[:n].copy()

    def result_range_doubles(self) -> int:
        return int(self._lib.msckf_result_range_doubles(self._h))

    def shared_result(self) -> UpdateResult:
        """The complete result of a sharded update as read from the result range (any rank, after the
        broadcast): status, dx, P+, accepted[F_total] of the whole batch in input order, gate counters."""
        d = 15 + 6 * self._N
        F = getattr(self, "_F_total", 0)
        dx, P_out = np.empty(d), np.empty((d, d))
        acc = np.zeros(max(F, 1), dtype=np.uint8)
        st = _ffi.Stats()
        rc = self._check(self._lib.msckf_get_shared_result(self._h, _ffi.dptr(dx), _ffi.dptr(P_out), _ffi.uptr(acc), C.byref(st)))
        return UpdateResult(rc, dx, P_out, acc[:F].copy(), st.as_dict())

    def result_device_view(self):
        """`dx | P+` of the last run as ONE contiguous HBM range (d + d*d doubles) exposed through
        `__cuda_array_interface__`: `torch.as_tensor(view, device="cuda")` wraps it without a copy, e.g. as the
        send buffer of the broadcast that follows the merge on rank 0.  Valid until the engine is closed; its
        contents change with every run (synchronise the engine's stream first)."""
        d = 15 + 6 * self._N
        ptr = int(self._lib.msckf_device_pointer(self._h, 0))

        class _View:
            __cuda_array_interface__ = {"shape": (d + d * d,), "typestr": "<f8", "data": (ptr, False), "version": 2}
        return _View()

    def export_result(self, dx_ptr: int, P_ptr: int):
        """dx and P+ of the last run into HBM buffers owned by the caller."""
        self._check(self._lib.msckf_export_result(self._h, C.c_void_p(dx_ptr), C.c_void_p(P_ptr), 1), allow_noop=False)

    def import_covariance(self, P):
        """New prior covariance from a host array or an int device address."""
        if isinstance(P, (int, np.integer)):
            self._check(self._lib.msckf_import_covariance(self._h, C.c_void_p(int(P)), 1), allow_noop=False)
        else:
            a = _ffi.f64(P)
            self._check(self._lib.msckf_import_covariance(self._h, a.ctypes.data_as(C.c_void_p), 0), allow_noop=False)

    # -- introspection ------------------------------------------------------
    def debug_gate(self):
        g = np.zeros(max(self._F, 1))
        q = np.zeros(max(self._F, 1), dtype=np.int32)
        self._check(self._lib.msckf_debug_gate(self._h, _ffi.dptr(g), _ffi.iptr(q)), allow_noop=False)
        return g[:self._F], q[:self._F]

    def debug_split(self) -> dict:
        """How the loaded batch's long tracks were planned (`msckf_debug_split`)."""
        out = (C.c_int32 * 8)()
        self._check(self._lib.msckf_debug_split(self._h, out), allow_noop=False)
        names = ("long_tracks", "narrow_blocks", "remainder_rows_cap", "remainder_mode", "remainder_tree_levels", "entries",
                 "band_plan", "sweep_mode")
        return dict(zip(names, [int(x) for x in out]))

    def set_rem_direct_rows(self, rows: int = -1):
        """Tests: remainder rows up to which K6-K7 takes them without a QR of their own (< 0: the default)."""
        self._check(self._lib.msckf_debug_set_rem_direct_rows(self._h, int(rows)), allow_noop=False)

    def debug_compressed(self):
        dc = 6 * self._N
        T = np.zeros((dc, dc))
        rn = np.zeros(dc)
        self._check(self._lib.msckf_debug_compressed(self._h, _ffi.dptr(T), _ffi.dptr(rn)), allow_noop=False)
        return T, rn

    # -- reference-shaped drop-in ---------------------------------------------
    def update(self, filt, features, view_sigma=None, point_priors=None) -> int:
        """Drop-in for `MSCKF.update(features)` (reference `MSCKF.py:570-609`)
        including `correct` (`:611-661`).  `filt` is any object with the
        attributes the reference method reads: `state.cameras` (ordered mapping
        key -> camera with `T_W_Ci`, `T_W_Ci_null`, each with `.R`, `.t`),
        `state.covariance`, `state.imu` (`W_gravity`, `T_W_Ii`, `v_W_Ii`,
        `gyroscope_bias`, `accelerometer_bias`), `K`, `sigma_image`,
        `number_of_residuals_discarded_for_gasting_test`.
        `view_sigma`: optional mapping feature key -> one standard deviation per view, in the order of
        `Feature.keypoints` and in `sigma_image`'s units (R_o = blockdiag(sigma_v^2 I_2) in place of `:589`; a
        feature the mapping does not name stays at `sigma_image`).  `None`: the reference's update.
        `point_priors`: optional mapping feature key -> (mean (3,), cov (3, 3)) of a known landmark in the world frame
        (`set_point_priors`); features it does not name are plain tracks.
        A robust loss needs no argument here: `set_robust` is a setting of the engine and this call honours it.
        Returns the status (0 updated / 1 no-op); mutates `filt` like the reference."""
        from .pack import point_priors_from_reference, problem_from_reference, view_sigma_from_reference
        from .inject import inject_state
        prob = problem_from_reference(filt, features)
        if view_sigma is not None:
            prob.view_sigma = view_sigma_from_reference(features, view_sigma, prob.sigma)
        if point_priors is not None:
            prob.point_prior = point_priors_from_reference(features, point_priors)
        res = self.update_problem(prob)
        filt.number_of_residuals_discarded_for_gasting_test += res.n_rejected        # MSCKF.py:578
        if res.status != 0:
            return res.status                                                         # MSCKF.py:584-585
        filt.state.covariance = res.P_new                                             # MSCKF.py:614 (rebinds)
        inject_state(filt.state, res.dx)                                              # MSCKF.py:616-661
        return 0

    def process_features(self, filt, view_sigma=None, refine_iters: int = 0, point_priors=None) -> int:
        """Drop-in for `MSCKF.process_features()` (reference `MSCKF.py:450-456`):
        `get_valid_features(self.features)` and `update(valid_features)` in one device pass,
        then `remove_features(lost_features)` through the filter's own method.  Mutates the
        features' inverse-depth points (`:488`) and the filter like the reference does.
        `view_sigma`, `point_priors`: as in `update`, keyed like `filt.features`.  The selection knows nothing of priors: a
        track it skips stays skipped, a refreshed point is where the prior track is linearised.
        `refine_iters`: 0 the reference's linear triangulation; 1..32 refines each triangulated point on the device
        under the current clone poses before the update (`run_select`); the features then carry the refined points.
        A robust loss set with `set_robust` stays in force (no argument here): its weights are formed at the refreshed points.
        Returns 0 updated / 1 no-op."""
        import dataclasses
        from .pack import (point_priors_from_reference, problem_from_reference, select_params_from_reference, tracks_from_reference,
                           view_sigma_from_reference)
        from .inject import inject_state
        feats = filt.features
        if len(feats) == 0:
            return 1
        prob = problem_from_reference(filt, feats)
        if view_sigma is not None:
            prob.view_sigma = view_sigma_from_reference(feats, view_sigma, prob.sigma)
        if point_priors is not None:
            prob.point_prior = point_priors_from_reference(feats, point_priors)
        self.load(prob)
        self.set_tracks(tracks_from_reference(feats))
        self.run_select(dataclasses.replace(select_params_from_reference(filt), refine_iters=int(refine_iters)), prob.K)
        sel = self.selection()
        if 0 < int(sel.valid.sum()) < 0.15 * len(feats):
            self.replan()                      # few valid candidates: a shallower QR tree pays for the sync
        self.run()
        res = self.result()
        items = list(feats.items())
        for j, (_, ft) in enumerate(items):
            if sel.flags[j] & _ffi.SEL_REFRESHED:                                     # MSCKF.py:488
                ft.inverse_depth_point.m = sel.idp_m[j].copy()
                ft.inverse_depth_point.rho = float(sel.idp_rho[j])
                if hasattr(filt, "estimated_world_points"):
                    filt.estimated_world_points.append(sel.world[j].copy())           # :489
        if not sel.valid.any():
            return 1                                                                  # :454
        filt.number_of_residuals_discarded_for_gasting_test += res.n_rejected        # :578
        if res.status == 0:
            filt.state.covariance = res.P_new                                         # :614
            inject_state(filt.state, res.dx)                                          # :616-661
        filt.remove_features({k: ft for j, (k, ft) in enumerate(items) if sel.flags[j] & _ffi.SEL_LOST})   # :456
        return res.status

    def prune_poorest_camera_states(self, filt, refine_iters: int = 0) -> int:
        """Drop-in for `MSCKF.prune_poorest_camera_states()` (reference `MSCKF.py:710-737`): the two clones seen by
        the fewest features, the features seen by them -> `get_valid_features` -> `update` -> `remove_cameras`,
        composed on the resident engine (`_prune`).  `refine_iters` as in `process_features`; `set_robust`, a setting of the
        engine, is honoured without an argument.  Returns 0 updated / 1 no update."""
        count = {}
        for ft in filt.features.values():                                             # :712-716
            for ci in ft.camera_indices:
                count[ci] = count.get(ci, 0) + 1
        poorest = [k for k, _ in sorted(count.items(), key=lambda kv: kv[1])][:2]     # :718-724 (stable sort, dict order)
        return self._prune(filt, {k: filt.state.cameras[k] for k in poorest}, refine_iters)

    def prune_camera_states(self, filt, refine_iters: int = 0) -> int:
        """Drop-in for `MSCKF.prune_camera_states()` (reference `MSCKF.py:663-680`): every
        `int(max_number_of_camera_states / camera_states_to_delete)`-th clone of the window (position i > 0 with
        i % step == 0, `:665-667`), the features seen by them -> `get_valid_features` -> `update` ->
        `remove_cameras`, composed on the resident engine (`_prune`).  `refine_iters` as in `process_features`; `set_robust`,
        a setting of the engine, is honoured without an argument.  Returns 0 updated / 1 no update."""
        step = int(filt.max_number_of_camera_states / filt.camera_states_to_delete)   # :666
        drop = {k: cam for i, (k, cam) in enumerate(filt.state.cameras.items()) if i > 0 and i % step == 0}
        return self._prune(filt, drop, refine_iters)

    def _prune(self, filt, drop, refine_iters: int = 0) -> int:
        """Shared tail of the reference's two pruning methods (`MSCKF.py:669-680`, `:726-737`): selection, update,
        commit and the removal of the clones' rows / columns (`:751-757`) run back to back in HBM; the covariance
        crosses PCIe once in each direction.  The dictionary bookkeeping of `remove_cameras` (`:758-777`, including
        the `last_camera_measurement` entries of features that lost all their views) stays on the host."""
        import dataclasses
        from .pack import problem_from_reference, select_params_from_reference, tracks_from_reference
        from .inject import inject_state
        cams = filt.state.cameras
        todo = {i: ft for i, ft in filt.features.items() if any(ci in drop for ci in ft.camera_indices)}   # :669-674
        keys = list(cams.keys())
        slots = [keys.index(k) for k in drop]
        status = 1
        if len(todo) > 0:
            prob = problem_from_reference(filt, todo)
            self.load(prob)
            self.set_tracks(tracks_from_reference(todo))
            self.run_select(dataclasses.replace(select_params_from_reference(filt), refine_iters=int(refine_iters)), prob.K)
            sel = self.selection()
            items = list(todo.items())
            for j, (_, ft) in enumerate(items):
                if sel.flags[j] & _ffi.SEL_REFRESHED:                                 # :488
                    ft.inverse_depth_point.m = sel.idp_m[j].copy()
                    ft.inverse_depth_point.rho = float(sel.idp_rho[j])
                    if hasattr(filt, "estimated_world_points"):
                        filt.estimated_world_points.append(sel.world[j].copy())
            if sel.valid.any():                                                       # :676-678
                self.run()
                d = 15 + 6 * self._N
                dx = np.zeros(d)
                acc = np.zeros(max(self._F, 1), dtype=np.uint8)
                st = _ffi.Stats()
                status = self._check(self._lib.msckf_get_result(self._h, _ffi.dptr(dx), None, _ffi.uptr(acc), C.byref(st)))
                filt.number_of_residuals_discarded_for_gasting_test += int(st.n_rejected)     # :578
                if status == 0:
                    self.commit_covariance()                                          # :614, P+ stays in HBM
                    inject_state(filt.state, dx)                                      # :616-661 (before the clones go)
        else:
            self.set_prior(filt.state.covariance, filt.state.imu.W_gravity, filt.K, filt.sigma_image,
                           [c.T_W_Ci.R for c in cams.values()], [c.T_W_Ci.t for c in cams.values()])
        if slots:
            self.remove_clones(slots)                                                 # :751-757 on the resident P
        filt.state.covariance = self.covariance()
        for k in drop:                                                                # :758
            del cams[k]
        gone = []
        for i, ft in filt.features.items():                                           # :760-769
            for k in drop:
                if k in ft.camera_indices:
                    v = ft.camera_indices.index(k)
                    for name in ("keypoints", "descriptors", "scores", "camera_indices", "lines"):
                        lst = getattr(ft, name, None)
                        if lst is not None and len(lst) > v:
                            del lst[v]
            if len(ft.camera_indices) == 0:
                gone.append(i)
        lcm = getattr(filt, "last_camera_measurement", None)
        for i in gone:                                                                # :771-777
            del filt.features[i]
            if lcm is not None:
                idx = np.where(lcm.features_indices == i)[0]
                if len(idx) > 0:
                    lcm.descriptors = np.delete(lcm.descriptors, idx[0], axis=0)
                    lcm.features_indices = np.delete(lcm.features_indices, idx[0], axis=0)
        return status
