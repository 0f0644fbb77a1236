"""The cases of tests/test_wide_store.py (CPU) and tests/test_gpu_wide_store.py: the track store of a context created with
`max_track` > 32 and `MSCKF_FLAG_WIDE_STORE` (`UpdateEngine(..., wide_store=True)`), whose rows hold up to 64 views and whose
per-row kernels (`k_track_emit<64>`, `k_track_drop<64>`, `k_track_frame<64>`) give a row a whole wavefront.

`window`, `grow`, `store_batch`, `host_door` and `same_through_both_doors` restate `_small`, `_grow`, `_store_batch`,
`_host_door` and `_same_through_both_doors` of tests/test_gpu_tracks.py for windows of more than 32 clones.  Every case is
seeded; windows are 34 to 66 clones, plus one of 100; stores hold at most 16 tracks.  What the GPU tests rely on -- where the
first failing view of a pair lies, that no gate is borderline, that no similarity is near a threshold -- is decided here
from the oracle and the NumPy restatements alone and asserted by the CPU file.  Not a conftest: imported by name."""
import functools

import numpy as np

import match_options_ref as mor
from msckf_amd import synth
from oracle import msckf_oracle as oracle

F64EPS = float(np.finfo(np.float64).eps)
INF = float("inf")
PARAMS = dict(min_frames_lost=1, min_frames_tracked=2, use_parallax=False, min_parallax_deg=0.0)

J15 = np.zeros((6, 15))
J15[0:3, 0:3] = np.eye(3)
J15[3:6, 12:15] = np.eye(3)


def wide_engine(**kw):
    """The engine under test: rows of 64 views."""
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=64, max_features=16, max_track=64, wide_store=True)
    args.update(kw)
    return UpdateEngine(**args)


def door_engine(**kw):
    """The host door: a wide-track context created WITHOUT the flag (tests/test_gpu_wide_tracks.py holds it to the oracle)."""
    from msckf_amd.api import UpdateEngine
    args = dict(max_clones=64, max_features=16, max_track=64)
    args.update(kw)
    return UpdateEngine(**args)


# ---- windows, stores and batches ------------------------------------------------------------------------------------------
def window(N, F, M, seed):
    """Synthetic poses and consistent keypoints: uv[j, s] is feature j's view in clone s, NaN where it has none (M < N: a
    track is seen in M consecutive clones)."""
    p = synth.make_problem(N, F, M, seed=seed)
    uv = np.full((F, N, 2), np.nan)
    for j in range(F):
        a, b = int(p.view_ptr[j]), int(p.view_ptr[j + 1])
        uv[j, np.asarray(p.obs_slot[a:b])] = np.asarray(p.obs_uv[a:b], dtype=np.float64)
    return p, uv


def small(N, F, seed):
    p, uv = window(N, F, N, seed)
    assert not np.isnan(uv).any()
    return p, uv


def confidences(views, N):
    """conf[j][k]: the score `grow` gives view k of track j (0.5 + 0.01 x its place in its clone's list)."""
    out = [[] for _ in views]
    for s in range(N):
        js = [j for j in range(len(views)) if s in views[j]]
        for k, j in enumerate(js):
            out[j].append(0.5 + 0.01 * k)
    return [np.array(c) for c in out]


def grow(eng, p, uv, views, ids, upto=None):
    """One clone at a time: `views[j]` lists the clones track ids[j] is seen in.  No view is tested (`tracks_observe`)."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((15, 15))
    eng.set_prior(A @ A.T / 15 + np.eye(15) * 0.1, p.gravity, p.K, p.sigma)
    for s in range(p.N if upto is None else upto):
        eng.augment(J15, p.cam_R[s], p.cam_t[s])
        js = [j for j in range(len(ids)) if s in views[j]]
        eng.tracks_observe([ids[j] for j in js], uv[js, s], 0.5 + 0.01 * np.arange(len(js)))


def store_batch(eng, ids):
    """The candidates as the store holds them, in the layout of `set_features` + `set_tracks`."""
    tr = [eng.track(int(i)) for i in ids]
    nv = [len(t["slots"]) for t in tr]
    cat = lambda k, w: np.concatenate([t[k].reshape(-1, w) for t in tr]) if tr else np.zeros((0, w))
    return tr, dict(view_ptr=np.concatenate([[0], np.cumsum(nv)]).astype(np.int32), obs_uv=cat("uv", 2),
                    obs_slot=np.concatenate([t["slots"] for t in tr]).astype(np.int32) if tr else np.zeros(0, np.int32),
                    line_base=cat("line_base", 3), line_dir=cat("dir", 3), line_conf=cat("conf", 1).reshape(-1),
                    idp_base=np.array([t["idp_base"] for t in tr]).reshape(-1, 3),
                    idp_m=np.array([t["idp_m"] for t in tr]).reshape(-1, 3), idp_rho=np.array([t["idp_rho"] for t in tr]))


def host_batch(p, uv, views):
    """The same layout from NumPy alone: what the reference's front end holds for these tracks (`MSCKF.py:403-434`): the
    direction R K^-1 [u, v, 1] of every view, the clone's position as its base, m = the first direction normalised, rho 0.1."""
    Kinv = np.linalg.inv(np.asarray(p.K, dtype=np.float64))
    conf = confidences(views, p.N)
    vp, ouv, slot, d, base, m = [0], [], [], [], [], []
    for j, vs in enumerate(views):
        for s in vs:
            ouv.append(uv[j, s])
            slot.append(s)
            d.append(p.cam_R[s] @ (Kinv @ np.append(uv[j, s], 1.0)))
        vp.append(len(slot))
        base.append(p.cam_t[vs[0]])
        m.append(d[vp[-2]] / np.linalg.norm(d[vp[-2]]))
    return dict(view_ptr=np.array(vp, np.int32), obs_uv=np.array(ouv).reshape(-1, 2), obs_slot=np.array(slot, np.int32),
                line_base=p.cam_t[np.array(slot, int)].reshape(-1, 3), line_dir=np.array(d).reshape(-1, 3), line_conf=np.concatenate(conf),
                idp_base=np.array(base).reshape(-1, 3), idp_m=np.array(m).reshape(-1, 3), idp_rho=np.full(len(views), 0.1))


def problem_of(b, P, cam_R, cam_t, gravity, K, sigma):
    return synth.UpdateProblem(P=P, cam_R=cam_R, cam_t=cam_t, cam_R0=cam_R, cam_t0=cam_t, gravity=gravity, K=K, sigma=sigma,
                               view_ptr=b["view_ptr"], obs_uv=b["obs_uv"], obs_slot=b["obs_slot"], idp_base=b["idp_base"],
                               idp_m=b["idp_m"].copy(), idp_rho=b["idp_rho"].copy())


def tracks_of(b, lost, tracked):
    return synth.TrackTable(line_base=b["line_base"], line_dir=b["line_dir"], line_conf=b["line_conf"],
                            lost_for=np.asarray(lost, np.int32), tracked_for=np.asarray(tracked, np.int32))


def host_door(eng_b, b, P, cam_R, cam_t, gravity, K, sigma, lost, tracked, params):
    """The batch `b` through `set_features` + `set_tracks` on a second engine holding the same state."""
    eng_b.set_prior(P, gravity, K, sigma, cam_R, cam_t)
    eng_b.set_features(problem_of(b, P, cam_R, cam_t, gravity, K, sigma))
    eng_b.set_tracks(tracks_of(b, lost, tracked))
    eng_b.run_select(params, K)
    sel = eng_b.selection()
    res = None
    if int(sel.valid.sum()):
        eng_b.run()
        res = eng_b.result()
    return sel, res


def same_through_both_doors(sel, res, sel_b, res_b, what):
    assert np.array_equal(sel.flags, sel_b.flags), what
    assert np.array_equal(sel.idp_m, sel_b.idp_m) and np.array_equal(sel.idp_rho, sel_b.idp_rho), what
    assert (res is None) == (res_b is None), what
    if res is not None:
        assert res.status == res_b.status and np.array_equal(res.accepted, res_b.accepted), what
        assert np.array_equal(res.dx, res_b.dx) and np.array_equal(res.P_new, res_b.P_new), what


def chained_reference(prob, flags, idp_m, idp_rho):
    """`oracle.update` on the tracks a selection took, fed that selection's inverse-depth points (as
    tests/test_gpu_wide_tracks.py holds its chained update).  (valid indices, oracle result)."""
    valid = np.nonzero(np.asarray(flags) & 1)[0]
    chained = prob.take(valid)
    chained.idp_m, chained.idp_rho = np.asarray(idp_m)[valid], np.asarray(idp_rho)[valid]
    return valid, oracle.update(chained, dense_noise=False)


# ---- 1: store batch = host batch -------------------------------------------------------------------------------------------
# name -> (clones, seed, ids, views).  w48: 31, 32, 33 and 48 views among 1, 2 and 10, and a track that skips every third
# clone; w64: 63 and 64 views, a track on slots 32..63 only, among 10, 2 and 1
UPDATE_CASES = {
    "w48": (48, 131, [14, 3, 27, 8, 41, 5, 19, 33],
            [list(range(0, 31)), list(range(5, 37)), list(range(10, 43)), list(range(0, 48)), [20], [3, 4], list(range(30, 40)),
             [s for s in range(48) if s % 3 != 1]]),
    "w64": (64, 132, [9, 2, 30, 11, 6, 21],
            [list(range(0, 63)), list(range(0, 64)), list(range(32, 64)), list(range(50, 60)), [7, 9], [63]]),
}


@functools.lru_cache(maxsize=None)
def update_case(name):
    """dict(p, uv, ids, views, lost, tracked, host (the NumPy batch), ref (select + chained update by the oracle))."""
    N, seed, ids, views = UPDATE_CASES[name]
    p, uv = small(N, len(ids), seed)
    lost, tracked = np.ones(len(ids), np.int32), np.array([len(v) for v in views], np.int32)
    host = host_batch(p, uv, views)
    prob = problem_of(host, p.P, p.cam_R, p.cam_t, p.gravity, p.K, p.sigma)
    sel = oracle.select_features(prob, tracks_of(host, lost, tracked), synth.SelectParams(**PARAMS))
    valid, ref = chained_reference(prob, sel["flags"], sel["idp_m"], sel["idp_rho"])
    return dict(p=p, uv=uv, ids=ids, views=views, lost=lost, tracked=tracked, host=host, sel=sel, valid=valid, ref=ref)


# ---- 4: frame intake ------------------------------------------------------------------------------------------------------
# A corridor of 63 clones in the store and a 64th, the newest, 1.5 mm and 2e-3 rad from clone FRAME_NEAR: a stored view of that
# clone is tested by the homography, every other by the signed epipolar score (`MSCKF.py:368, :392`).  A track's keypoint in
# the newest clone is its keypoint in clone FRAME_NEAR mapped through K R_new^T R_near K^-1 (the parallax of 1.5 mm at 4 m and
# more is below the pixel noise).  The thresholds lie above every honest view's score; a failure is placed at view k by storing
# a displaced keypoint there through `tracks_observe`, which does not test.
FRAME_N, FRAME_NEAR, FRAME_SEED = 63, 40, 141
THR_E, THR_H = 3.0, 5.0           # (the epipolar score x2^T F x1 is signed and not small on an honest pair: MSCKF.py:392-393)
FRAME_SEPARATION = 3.0            # every honest score lies below thr / 3 and every displaced one above 3 thr
FRAME_PUSH = 10.0                 # a displaced keypoint's epipolar score, in thresholds
# (id, slots, the view that fails or None, 1 epipolar / 2 homography)
FRAME_TRACKS = [
    (101, [62], None, 0), (102, list(range(0, 31)), None, 0), (103, list(range(31, 63)), None, 0), (104, list(range(0, 33)), None, 0),
    (105, list(range(0, 63)), None, 0),
    (111, [5], 0, 1), (112, list(range(0, 31)), 30, 1), (113, list(range(20, 52)), 31, 1), (114, list(range(30, 63)), 0, 1),
    (115, list(range(0, 33)), 31, 1), (116, list(range(0, 33)), 32, 1), (117, list(range(0, 63)), 10, 1), (118, list(range(0, 63)), 62, 1),
    (121, list(range(8, 41)), 32, 2), (122, list(range(0, 63)), 40, 2),
]
# a second displaced view behind the first, on the other side of bit 32 of the row's ballot: the FIRST failure decides, and its
# kind is read at that bit (117: epipolar at 10, then homography at 40; 122: homography at 40, then epipolar at 50)
FRAME_LATER = {117: (40, 2), 122: (50, 1)}
FRAME_FRESH = 130                 # an id the store does not know rides in the same call
FRAME_FULL = 105                  # holds 64 views after the frame: the next pair on it is refused


def _pair_scores(K, pose1, pose2, fk, mk):
    """(branch, score, d score / d fk) of one (stored view, new keypoint) test as `oracle.associate` forms it: branch 2 the
    homography score, 1 the signed epipolar score, which is linear in the stored keypoint fk."""
    invK = np.linalg.inv(K)
    T1, T2 = np.eye(4), np.eye(4)
    T1[:3, :3], T1[:3, 3] = pose1
    T2[:3, :3], T2[:3, 3] = pose2
    T12 = np.linalg.inv(T1) @ T2
    R12, t12 = T12[:3, :3], T12[:3, 3]
    if np.linalg.norm(t12) < 0.01:
        H = K @ R12 @ invK
        x1 = np.linalg.inv(H) @ np.append(mk, 1.0)
        x2 = H @ np.append(fk, 1.0)
        return 2, (np.linalg.norm(mk - x1[:2] / x1[2]) + np.linalg.norm(fk - x2[:2] / x2[2])) / 2, None
    a = np.append(mk, 1.0) @ (invK.T @ oracle.skew(t12) @ R12 @ invK)
    return 1, float(a @ np.append(fk, 1.0)), a[:2]


@functools.lru_cache(maxsize=None)
def frame_case():
    p, uv = small(FRAME_N, len(FRAME_TRACKS), FRAME_SEED)
    K = np.asarray(p.K, dtype=np.float64)
    rng = np.random.default_rng(FRAME_SEED)
    R_new = synth.so3_exp(2e-3 * rng.standard_normal(3)) @ p.cam_R[FRAME_NEAR]
    off = rng.standard_normal(3)
    t_new = p.cam_t[FRAME_NEAR] + 1.5e-3 * off / np.linalg.norm(off)
    H = K @ R_new.T @ p.cam_R[FRAME_NEAR] @ np.linalg.inv(K)
    new_uv = np.array([(lambda x: x[:2] / x[2])(H @ np.append(uv[j, FRAME_NEAR], 1.0)) for j in range(len(FRAME_TRACKS))])
    stored = uv.copy()
    honest, displaced = [], []
    for j, (i, slots, first, first_kind) in enumerate(FRAME_TRACKS):
        bad = ([(first, first_kind)] if first is not None else []) + ([FRAME_LATER[i]] if i in FRAME_LATER else [])
        for k, kind in bad:
            s = slots[k]
            b, x, a = _pair_scores(K, (p.cam_R[s], p.cam_t[s]), (R_new, t_new), uv[j, s], new_uv[j])
            assert b == kind, (j, b)
            if kind == 1:             # along the score's gradient, to FRAME_PUSH thresholds
                stored[j, s] = uv[j, s] + a * (FRAME_PUSH * THR_E - x) / (a @ a)
            else:                     # (the score measures how far H moves a point: far outside the image it moves it far)
                stored[j, s] = uv[j, s] + np.array([3000.0, -2000.0])
            displaced.append(_pair_scores(K, (p.cam_R[s], p.cam_t[s]), (R_new, t_new), stored[j, s], new_uv[j])[1] / (THR_E if kind == 1 else THR_H))
        for v, s in enumerate(slots):
            if v not in [k for k, _ in bad]:
                b, x, _ = _pair_scores(K, (p.cam_R[s], p.cam_t[s]), (R_new, t_new), stored[j, s], new_uv[j])
                honest.append(x / (THR_E if b == 1 else THR_H))
    ids = [t[0] for t in FRAME_TRACKS]
    views = [t[1] for t in FRAME_TRACKS]
    host = host_batch(p, stored, views)
    P = synth.random_spd_covariance(15 + 6 * FRAME_N, rng)
    prob = problem_of(host, P, p.cam_R, p.cam_t, p.gravity, p.K, p.sigma)
    res, fail = oracle.associate(prob, new_uv, R_new, t_new, p.K, THR_E, THR_H)
    return dict(p=p, uv=stored, ids=ids, views=views, new_uv=new_uv, R_new=R_new, t_new=t_new, prob=prob, res=res, fail=fail,
                honest=float(np.max(honest)), displaced=float(np.min(displaced)),
                score=np.random.default_rng(FRAME_SEED + 1).uniform(0.2, 1.0, len(ids) + 1))


# ---- 3, 5: stores fed by descriptors ---------------------------------------------------------------------------------------
DESC_D, MIN_COS = 32, 0.8
RADIUS, MARGIN = 40.0, 0.05


def walk_frames(uv, views, N, seed, D=DESC_D):
    """One frame per clone: (keypoints, descriptors fp32, scores, the tracks they belong to) in shuffled order.  Track j's
    descriptor is a unit vector of its own plus 5 % noise per view."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((len(views), D))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    out = []
    for s in range(N):
        js = np.array([j for j in range(len(views)) if s in views[j]], dtype=int)
        js = js[rng.permutation(len(js))]
        d = a[js] + 0.05 * rng.standard_normal((len(js), D)) / np.sqrt(D)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append((uv[js, s].reshape(-1, 2), d.astype(np.float32), rng.uniform(0.3, 1.0, len(js)), js))
    return out


def walk_model(p, frames, radius=0.0, margin=0.0, upto=None):
    """The restatement (tests/match_options_ref.py; with both options 0 it is tests/match_ref.py's rule) fed the frames, its
    guards on: every similarity GUARD from a threshold or a runner-up.  Returns (store, per frame None where the reference
    returns early -- no keypoint, or no pair matched: nothing changes -- else (ids, result, why or None, table ids or None,
    similarity per keypoint))."""
    st = mor.Store(p.K, MIN_COS, INF, INF, radius, margin, guarded=True)
    log = []
    for s, (kp, d, sc, _) in enumerate(frames[:upto]):
        st.add_camera(s, p.cam_R[s], p.cam_t[s])
        table_ids = list(st.table_ids)
        out = st.intake(s, kp, d, sc)
        if out is None:
            log.append(None)
            continue
        ids, res, pairs = out
        sim = np.zeros(len(kp))
        if st.last is not None:
            sim[st.last.idx2] = st.last.S[st.last.idx1, st.last.idx2]
        log.append((ids, res, None if st.last is None else st.last.why.copy(), None if st.last is None else table_ids, sim))
    return st, log


# 3: a 64-view track over slots 0..63 among shorter ones (ids are the model's: 1, 2, ... in the order of creation)
DROP_N, DROP_SEED = 64, 151
DROP_VIEWS = [list(range(0, 64)), list(range(0, 10)), list(range(40, 64)), [31, 32], [63], list(range(20, 45))]
DROP_SETS = {
    "first": [0], "last_of_the_lower_half": [31], "first_of_the_upper_half": [32], "last": [63],
    "the_four_corners": [0, 31, 32, 63], "upper_half": list(range(32, 64)), "lower_half_and_the_anchor": list(range(0, 32)),
    "every_clone_of_a_track": list(range(20, 45)),
}
DROP100_N, DROP100_FIRST, DROP100_SET = 100, 36, [36, 67, 68, 99]


@functools.lru_cache(maxsize=None)
def drop_case():
    p, uv = small(DROP_N, len(DROP_VIEWS), DROP_SEED)
    return dict(p=p, uv=uv, views=DROP_VIEWS, frames=walk_frames(uv, DROP_VIEWS, DROP_N, DROP_SEED))


@functools.lru_cache(maxsize=None)
def drop100_case():
    """A window of 100 clones; track 0 lies on slots 36..99 (the first seed whose first track starts there)."""
    for seed in range(2000, 2400):
        if int(synth.make_problem(DROP100_N, 1, 64, seed=seed).obs_slot[0]) == DROP100_FIRST:
            break
    else:
        raise AssertionError("no seed puts the first track on slot %d" % DROP100_FIRST)
    p, uv = window(DROP100_N, 3, 64, seed)
    first = [int(p.obs_slot[p.view_ptr[j]]) for j in range(3)]
    assert first[0] == DROP100_FIRST
    views = [list(range(36, 100)), list(range(first[1], first[1] + 64, 2)), list(range(first[2] + 10, first[2] + 20))]
    return dict(p=p, uv=uv, views=views, frames=walk_frames(uv, views, DROP100_N, seed))


# 5: tracks of 33 to 40 views (and three short ones) on a window of 41 clones
MATCH_N, MATCH_SEED = 41, 161
MATCH_VIEWS = [list(range(0, 33 + k)) for k in range(8)] + [list(range(10, 30)), list(range(35, 41)), [0, 1, 2]]
MATCH_MODES = {"plain": (0.0, 0.0), "window_and_margin": (RADIUS, MARGIN)}


@functools.lru_cache(maxsize=None)
def match_case():
    p, uv = small(MATCH_N, len(MATCH_VIEWS), MATCH_SEED)
    return dict(p=p, uv=uv, views=MATCH_VIEWS, frames=walk_frames(uv, MATCH_VIEWS, MATCH_N, MATCH_SEED))


# ---- 6: a short run with the nominal state resident ------------------------------------------------------------------------
# A camera that looks and moves along world +x at 0.15 m per frame with a small yaw, two IMU samples per frame; twelve points
# ahead of it, in the image over the whole run.  Track id -> (first frame, last frame): a track that ends is lost in the next
# frame and becomes a candidate then, with more than 32 views at frames 34, 36, 38, 39 (the prune) and 43.
RUN_FRAMES, RUN_SIGMA, RUN_SEED = 45, 0.01, 61
RUN_TRACKS = {1: (0, 33), 2: (0, 35), 3: (2, 35), 4: (0, 37), 5: (5, 37), 6: (30, 33), 7: (33, 35), 8: (20, 37),
              9: (0, 38), 10: (0, 42), 11: (0, 44), 12: (3, 44)}
RUN_PRUNE_AT, RUN_PRUNE = 39, [0, 1, 17, 37]      # at 40 clones, a removal shaped like prune_poorest_camera_states'


def run_frames(eng):
    """Drives `eng` through the run: before each yield, the frame's IMU samples and its clone (`propagate_imu`,
    `augment_imu`).  Yields (frame, nominal() behind the augmentation, the ids seen, their keypoints in the newest clone, their
    scores).  What the caller does between two yields -- intake, update, injection, removals -- is the caller's."""
    rng = np.random.default_rng(RUN_SEED)
    K, g = synth.K_DEFAULT.copy(), synth.GRAVITY_DEFAULT.copy()
    pts = {i: np.array([rng.uniform(12.0, 18.0), rng.uniform(-2.0, 2.0), rng.uniform(-1.5, 1.5)]) for i in RUN_TRACKS}
    eng.set_prior(np.diag([1e-4] * 3 + [1e-6] * 3 + [1e-3] * 3 + [1e-5] * 3 + [1e-3] * 3), g, K, RUN_SIGMA)
    eng.set_nominal(np.eye(3), np.zeros(3), np.array([1.5, 0.0, 0.0]), g, np.eye(12) * 1e-5,
                    T_I_C=(synth.R_WC_DEFAULT, np.array([0.05, 0.0, 0.02])))
    for f in range(RUN_FRAMES):
        gyro = np.tile([0.0, 0.0, 0.02 * np.sin(0.4 * f)], (2, 1)) + 1e-4 * rng.standard_normal((2, 3))
        acc = np.tile(g, (2, 1)) + 1e-3 * rng.standard_normal((2, 3))      # R acc - g (IMU.py:94): no acceleration but the noise
        eng.propagate_imu(gyro, acc, np.full(2, 0.05))
        eng.augment_imu()
        nom = eng.nominal()
        R, t = nom["cam_R"][-1], nom["cam_t"][-1]
        seen = [i for i, (a, b) in RUN_TRACKS.items() if a <= f <= b]
        q = np.array([R.T @ (pts[i] - t) for i in seen])
        assert (q[:, 2] > 1.0).all()
        px = (q @ K.T)[:, :2] / q[:, 2:3] + 0.2 * rng.standard_normal((len(seen), 2))
        yield f, nom, seen, px, rng.uniform(0.3, 1.0, len(seen))
