#!/usr/bin/env python3
"""Generate `match/match_frames.npz`: twelve frames through the REFERENCE's own `add_camera_measurements`,
`remove_features` and `remove_cameras` (`MSCKF.py:268-444`, `:739-779`) with its own `FeatureExtractor.match` around a
NumPy `XFeat.match`.

The reference's matcher lives in a submodule that is not part of the reference checkout, so the
12-line rule is stated in `tests/match_ref.py` and plugged in here; everything around it is the reference's code.  Like
`gen_golden.py` (whose stub recipe, SURVEY.md Appendix A, this imports) it runs only where the reference is mounted, and
writes arrays only.  (The fixture sits in a directory of its own: every `golden/*.npz` is read as an update problem.)

    python tests/golden/gen_match_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden  # noqa: E402,F401  (the stub modules and the reference on sys.path)
from gen_golden import MSCKF, MSCKFParameters, Camera, Isometry3D  # noqa: E402
from src.msckf.FeatureExtractor import ExtractedFeature  # noqa: E402

import match_ref  # noqa: E402

D, N_FRAMES, MAX_KP = 8, 12, 60
MIN_COS, THR_E, THR_H = 0.82, 5e-3, 2.0
K = np.array([[400.0, 0.0, 320.0], [0.0, 400.0, 240.0], [0.0, 0.0, 1.0]])
PRUNE_AFTER, NO_MATCH, REMOVE_LOST_AFTER, EMPTY_AFTER, NEAR = 3, 5, 6, 8, 7      # NEAR: 3 mm from the frame before (homography tests)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def xfeat_match(d1, d2, min_cossim=0.82):
    """XFeat.match as `match_ref.match` states it; FeatureExtractor.match hands in torch tensors."""
    idx1, idx2, _ = match_ref.match(d1.numpy(), d2.numpy(), min_cossim)
    return idx1, idx2


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def make_frames(seed):
    rng = np.random.default_rng(seed)
    P = 72
    base = unit(rng.standard_normal((P, D)))
    for p in range(0, 16, 2):                                        # eight pairs of look-alike landmarks
        base[p + 1] = unit(base[p] + 0.15 * rng.standard_normal(D))
    pts = np.column_stack([rng.uniform(-3, 5, P), rng.uniform(-2, 2, P), rng.uniform(5, 10, P)])
    frames = []
    t = np.zeros(3)
    for f in range(N_FRAMES):
        t = t + (np.array([3e-3, 0.0, 0.0]) if f == NEAR else np.array([0.15, 0.01 * rng.standard_normal(), 0.02]))
        R = rot_y(0.01 * f)
        cam = (pts - t) @ R                                           # R^T (p - t), row-wise
        px = (K @ cam.T).T
        px = px[:, :2] / px[:, 2:3]
        vis = np.nonzero((px[:, 0] > 5) & (px[:, 0] < 635) & (px[:, 1] > 5) & (px[:, 1] < 475))[0]
        if f == NO_MATCH:
            sel = rng.choice(vis, 6, replace=False)
            desc = unit(-base[sel] + 0.08 * rng.standard_normal((6, D)))
        else:
            sel = rng.permutation(rng.choice(vis, min(len(vis), int(rng.integers(40, 56))), replace=False))
            noise = np.full(len(sel), 0.08)
            noise[rng.choice(len(sel), 3, replace=False)] = 0.35     # three keypoints whose descriptors drifted
            desc = unit(base[sel] + noise[:, None] * rng.standard_normal((len(sel), D)))
        kp = px[sel] + 0.3 * rng.standard_normal((len(sel), 2))
        wrong = rng.uniform(size=len(sel)) < 0.1
        kp[wrong] += rng.uniform(30, 60, (int(wrong.sum()), 2)) * rng.choice([-1.0, 1.0], (int(wrong.sum()), 2))
        assert len(sel) <= MAX_KP
        frames.append(dict(key=10 * (f + 1), R=R, t=t.copy(), kp=kp, desc=desc.astype(np.float32), score=rng.uniform(0.6, 1.0, len(sel))))
    return frames


def snapshot(f, tag, out, p):
    ids = list(f.features)
    keys = [list(f.features[i].camera_indices) for i in ids]
    out[p + tag + "_ids"] = np.array(ids, dtype=np.int32)
    out[p + tag + "_ptr"] = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int32)
    out[p + tag + "_keys"] = np.array([k for ks in keys for k in ks], dtype=np.int32)
    out[p + tag + "_lost"] = np.array([f.features[i].lost_for_n_frames for i in ids], dtype=np.int32)
    out[p + tag + "_tracked"] = np.array([f.features[i].tracked_for_n_frames for i in ids], dtype=np.int32)
    out[p + tag + "_desc"] = np.array([d for i in ids for d in f.features[i].descriptors], dtype=np.float32).reshape(-1, D)
    lcm = f.last_camera_measurement
    out[p + tag + "_table"] = np.asarray(lcm.descriptors, dtype=np.float64).reshape(-1, D)
    out[p + tag + "_table_ids"] = np.asarray(lcm.features_indices, dtype=np.int32).reshape(-1)


def score_margin(store, key, pairs, kps):
    """The smallest distance of a tested view's score from its threshold (the reference breaks at the first failure)."""
    Kinv = np.linalg.inv(K)
    worst = np.inf
    for i, j in pairs:
        tr = store.tracks[store.table_ids[i]]
        for v in range(len(tr.uv)):
            T1, T2 = np.eye(4), np.eye(4)
            T1[:3, :3], T1[:3, 3] = store.cams[tr.keys[v]]
            T2[:3, :3], T2[:3, 3] = store.cams[key]
            T12 = np.linalg.inv(T1) @ T2
            if np.linalg.norm(T12[:3, 3]) < 0.01:
                H = K @ T12[:3, :3] @ Kinv
                x1 = np.linalg.inv(H) @ np.append(kps[j], 1.0)
                x2 = H @ np.append(tr.uv[v], 1.0)
                s = (np.linalg.norm(kps[j] - x1[:2] / x1[2]) + np.linalg.norm(tr.uv[v] - x2[:2] / x2[2])) / 2
                worst = min(worst, abs(s - THR_H) / THR_H)
                if s > THR_H:
                    break
            else:
                F = Kinv.T @ match_ref._skew(T12[:3, 3]) @ T12[:3, :3] @ Kinv
                s = np.append(kps[j], 1.0) @ F @ np.append(tr.uv[v], 1.0)
                worst = min(worst, abs(s - THR_E) / THR_E)
                if s > THR_E:
                    break
    return worst


def run(seed):
    frames = make_frames(seed)
    params = MSCKFParameters()
    params.K = K
    params.min_cosine_similarity = MIN_COS
    params.epipolar_rejection_threshold = THR_E
    params.homography_rejection_threshold = THR_H
    f = MSCKF(params)
    f.feature_extractor.xfeat.match = xfeat_match
    f.current_image = np.zeros((4, 4, 3), dtype=np.uint8)
    f.state.covariance = np.zeros((15, 15))
    shadow = match_ref.Store(K, MIN_COS, THR_E, THR_H)               # only to name the failing test of each pair and the margins
    out = dict(n_frames=np.int32(N_FRAMES), K=K, desc_dim=np.int32(D), params=np.array([MIN_COS, THR_E, THR_H]))
    codes = set()
    for k, fr in enumerate(frames):
        p = f"f{k}_"
        key = fr["key"]
        n = f.state.covariance.shape[0]
        cov = np.zeros((n + 6, n + 6))
        cov[:n, :n] = f.state.covariance
        f.state.covariance = cov
        f.state.cameras[key] = Camera(K, 640, 480, Isometry3D(fr["R"].copy(), fr["t"].copy()))
        f.state.imu.id = key
        shadow.add_camera(key, fr["R"], fr["t"])
        for name in ("R", "t", "kp", "desc", "score"):
            out[p + name] = fr[name]
        out[p + "key"] = np.int32(key)
        had = len(f.features)
        if had:                                                      # the guards, on the table the reference is about to match
            A = np.asarray(f.last_camera_measurement.descriptors)
            g = match_ref.guards(A, fr["desc"], MIN_COS, need_pairs=k != NO_MATCH)
            assert (g["pairs"] == 0) == (k == NO_MATCH)
        before = {i: len(ft.camera_indices) for i, ft in f.features.items()}
        last0 = f.last_feature_index
        ne0, nh0 = f.number_of_features_discarded_for_epipolar_test, f.number_of_features_discarder_for_homography_test
        margin = np.inf
        if had and k != NO_MATCH:
            idx1, idx2, _ = match_ref.match(shadow.table, fr["desc"], MIN_COS)
            margin = score_margin(shadow, key, list(zip(idx1.tolist(), idx2.tolist())), fr["kp"])
            assert margin > 1e-3, margin
        f.add_camera_measurements(np.zeros((4, 4, 3), dtype=np.uint8),
                                  ExtractedFeature(keypoints=[x.copy() for x in fr["kp"]], descriptors=[x.copy() for x in fr["desc"]],
                                                   scores=[float(s) for s in fr["score"]]))
        sh = shadow.intake(key, fr["kp"], fr["desc"], fr["score"])
        skipped = len(f.features) == had and f.last_feature_index == last0 and all(len(f.features[i].camera_indices) == before[i] for i in before)
        assert skipped == (sh is None) == (k == NO_MATCH)
        out[p + "skipped"] = np.bool_(skipped)
        if not skipped:
            ids, res, pairs = sh
            # the shadow only names things: ids, appended views and both rejection counters are the reference's
            assert list(shadow.tracks) == list(f.features)
            for j in range(len(ids)):
                ft = f.features[int(ids[j])]
                appended = ft.camera_indices[-1] == key and np.array_equal(ft.keypoints[-1], fr["kp"][j])
                assert appended == (res[j] in (0, 4)), (k, j)
                assert (res[j] == 4) == (int(ids[j]) > last0)
            assert f.number_of_features_discarded_for_epipolar_test - ne0 == int((res == 1).sum())
            assert f.number_of_features_discarder_for_homography_test - nh0 == int((res == 2).sum())
            out[p + "ids"], out[p + "result"], out[p + "pairs"] = ids, res, pairs.astype(np.int32)
            codes |= set(res.tolist())
        out[p + "last_id"] = np.int32(f.last_feature_index)
        snapshot(f, "in", out, p)
        # what the frame's own removals do
        cams0 = list(f.state.cameras)
        rm_tracks, rm_keys = [], []
        if k == PRUNE_AFTER:
            rm_keys = [cams0[0], cams0[2]]
            f.remove_cameras({c: f.state.cameras[c] for c in rm_keys})
        elif k == REMOVE_LOST_AFTER:
            rm_tracks = [i for i, ft in f.features.items() if ft.lost_for_n_frames >= 2]
            assert len(rm_tracks) >= 3
            f.remove_features({i: f.features[i] for i in rm_tracks})
        elif k == EMPTY_AFTER:
            rm_tracks = list(f.features)
            f.remove_features({i: f.features[i] for i in rm_tracks})
            assert not f.features
        gone_keys = [c for c in cams0 if c not in f.state.cameras]
        ids0 = set(shadow.tracks)
        shadow.remove_tracks(rm_tracks)
        dropped = shadow.remove_cameras(gone_keys)
        assert list(shadow.tracks) == list(f.features) and ids0 - set(shadow.tracks) == set(rm_tracks) | set(dropped)
        out[p + "rm_tracks"] = np.array(rm_tracks, dtype=np.int32)
        out[p + "rm_keys"] = np.array(gone_keys, dtype=np.int32)
        out[p + "dropped"] = np.array(sorted(dropped), dtype=np.int32)
        if k == PRUNE_AFTER:
            assert dropped and any(len(ft.camera_indices) < before.get(i, 0) for i, ft in f.features.items())
        snapshot(f, "out", out, p)
    assert codes == {0, 1, 2, 4}, codes
    return out


def main():
    for seed in range(400):
        try:
            out = run(seed)
        except AssertionError as e:
            print(f"seed {seed}: {e!r}"[:160], flush=True)
            continue
        os.makedirs(os.path.join(HERE, "match"), exist_ok=True)
        path = os.path.join(HERE, "match", "match_frames.npz")
        out["seed"] = np.int32(seed)
        np.savez_compressed(path, **out)
        print(f"match_frames: seed {seed}, {os.path.getsize(path) / 1024:.0f} KiB")
        return
    raise SystemExit("no seed met the guards")


if __name__ == "__main__":
    main()
