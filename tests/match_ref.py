"""A NumPy restatement of the front end's frame intake from descriptors: the matching rule the engine runs on the device and
the bookkeeping of the reference's `add_camera_measurements` (`MSCKF.py:268-444`), `remove_features` and `remove_cameras`
(`:739-779`) around it.  `golden/match/match_frames.npz` holds what the reference itself did with the same frames;
`test_match_host.py` shows that this restatement reproduces it, and `test_gpu_tracks_match.py` holds the engine to both.

The rule (XFeat.match, mutual nearest neighbour).  A: the table, T x D, rows in the order the tracks were created; B: the
frame, n x D.  S = A B^T without normalisation; m12[i] = argmax_j S[i, j], m21[j] = argmax_i S[i, j], ties to the lowest
index; (i, m12[i]) is a match iff m21[m12[i]] == i and S[i, m12[i]] > min_cosine_similarity (strict)."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match", "match_frames.npz")
GUARD = 1e-4


def similarity(A, B):
    """S in fp64 from the fp32 values of both operands."""
    return np.asarray(A, dtype=np.float32).astype(np.float64) @ np.asarray(B, dtype=np.float32).astype(np.float64).T


def match(A, B, min_cos):
    """(idx1, idx2, S): the matched table rows (ascending) and their keypoints."""
    S = similarity(A, B)
    if S.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), S
    m12, m21 = np.argmax(S, axis=1), np.argmax(S, axis=0)          # np.argmax: the first of equal maxima
    i = np.arange(S.shape[0])
    ok = (m21[m12] == i) & (S[i, m12] > min_cos)
    return i[ok], m12[ok], S


def guards(A, B, min_cos, need_pairs=True):
    """What makes a frame a fair test of a matcher whose sums are rounded differently: every best similarity GUARD away
    from its runner-up (both directions) and from the threshold, and -- where the frame is meant to match -- a quarter of
    the table matched, a pair that fails mutuality alone and one that fails the threshold alone.  Returns a dict of the
    figures; raises AssertionError."""
    idx1, idx2, S = match(A, B, min_cos)
    T, n = S.shape
    out = dict(T=T, n=n, pairs=len(idx1))
    for M in (S, S.T):
        if M.shape[1] > 1:
            top = np.sort(M, axis=1)[:, -2:]
            gap = float((top[:, 1] - top[:, 0]).min())
            assert gap >= GUARD, ("runner-up", gap)
    best = S.max(axis=1)
    assert float(np.abs(best - min_cos).min()) >= GUARD, "threshold"
    assert float(np.abs(S.max(axis=0) - min_cos).min()) >= GUARD, "threshold"
    m12, m21 = np.argmax(S, axis=1), np.argmax(S, axis=0)
    mutual = m21[m12] == np.arange(T)
    out["only_mutuality"] = int((~mutual & (best > min_cos)).sum())
    out["only_threshold"] = int((mutual & ~(best > min_cos)).sum())
    if need_pairs:
        assert 4 * len(idx1) >= T, ("a quarter of the rows", len(idx1), T)
        assert out["only_mutuality"] >= 1 and out["only_threshold"] >= 1, out
    return out


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def view_test(K, invK, pose1, pose2, fk, mk, thr_e, thr_h):
    """One (stored view, new keypoint) test of `MSCKF.py:346-397`: 0 passed, 1 epipolar failure, 2 homography failure."""
    T1, T2 = np.eye(4), np.eye(4)
    T1[:3, :3], T1[:3, 3] = pose1
    T2[:3, :3], T2[:3, 3] = pose2
    T12 = np.linalg.inv(T1) @ T2
    R12, t12 = T12[:3, :3], T12[:3, 3]
    if np.linalg.norm(t12) < 0.01:
        H = K @ R12 @ invK
        x1 = np.linalg.inv(H) @ np.array([mk[0], mk[1], 1.0])
        x1 = x1[:2] / x1[2]
        x2 = H @ np.array([fk[0], fk[1], 1.0])
        x2 = x2[:2] / x2[2]
        return 2 if (np.linalg.norm(mk - x1) + np.linalg.norm(fk - x2)) / 2 > thr_h else 0
    F = invK.T @ _skew(t12) @ R12 @ invK
    return 1 if np.append(mk, 1.0) @ F @ np.append(fk, 1.0) > thr_e else 0


class Track:
    def __init__(self):
        self.uv, self.desc, self.score, self.keys = [], [], [], []
        self.lost = self.tracked = 0


class Store:
    """The front end's tracks and its `last_camera_measurement` table."""

    def __init__(self, K, min_cos, thr_e, thr_h):
        self.K = np.asarray(K, dtype=np.float64)
        self.min_cos, self.thr_e, self.thr_h = float(min_cos), float(thr_e), float(thr_h)
        self.tracks = {}                  # id -> Track, in creation order
        self.cams = {}                    # clone key -> (R, t)
        self.table_ids = []               # the table: one row per track, a snapshot
        self.table = np.zeros((0, 0), dtype=np.float32)
        self.last_id = 0

    def add_camera(self, key, R, t):
        self.cams[key] = (np.array(R, dtype=np.float64), np.array(t, dtype=np.float64))

    def _create(self, key, kp, d, s):
        self.last_id += 1
        tr = Track()
        tr.uv.append(kp); tr.desc.append(d); tr.score.append(s); tr.keys.append(key)
        tr.tracked = 1
        self.tracks[self.last_id] = tr
        return self.last_id

    def intake(self, key, keypoints, descriptors, scores):
        """One frame (already past the score floor).  Returns None where the reference returns early, else (ids, result,
        pairs): per keypoint the track it went to or created and the code 0 / 1 / 2 / 4, and the (table row, keypoint)
        pairs of the match."""
        kps = np.asarray(keypoints, dtype=np.float64).reshape(-1, 2)
        desc = np.asarray(descriptors, dtype=np.float32)
        n = len(kps)
        if n == 0:
            return None
        ids, res = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        if not self.tracks:
            for j in range(n):
                ids[j], res[j] = self._create(key, kps[j], desc[j], float(scores[j])), 4
            self.table_ids = list(self.tracks)
            self.table = desc.copy()                                  # raw rows (:311)
            return ids, res, np.zeros((0, 2), dtype=np.int64)
        idx1, idx2, _ = match(self.table, desc, self.min_cos)
        if len(idx1) == 0:
            return None                                               # :320
        invK = np.linalg.inv(self.K)
        matched_rows = set(idx1.tolist())
        lost_ids = [self.table_ids[i] for i in range(len(self.table_ids)) if i not in matched_rows]
        for i, j in zip(idx1.tolist(), idx2.tolist()):
            tid = self.table_ids[i]
            tr = self.tracks[tid]
            ids[j] = tid
            code = 0
            for v in range(len(tr.uv)):
                code = view_test(self.K, invK, self.cams[tr.keys[v]], self.cams[key], tr.uv[v], kps[j], self.thr_e, self.thr_h)
                if code:
                    break
            res[j] = code
            if code:
                tr.lost += 1
                continue
            tr.uv.append(kps[j]); tr.desc.append(desc[j]); tr.score.append(float(scores[j])); tr.keys.append(key)
            tr.tracked += 1
            tr.lost = 0
        taken = set(idx2.tolist())
        for j in range(n):
            if j not in taken:
                ids[j], res[j] = self._create(key, kps[j], desc[j], float(scores[j])), 4
        rows = []
        for tid, tr in self.tracks.items():
            if tid in lost_ids:
                tr.lost += 1
            w = np.asarray(tr.score, dtype=np.float64)
            d = np.asarray(tr.desc, dtype=np.float32).astype(np.float64)
            acc, den = np.zeros(d.shape[1]), 0.0
            for v in range(len(w)):                                   # in view order
                acc = acc + d[v] * w[v]
                den = den + w[v]
            rows.append((acc / den).astype(np.float32))
        self.table_ids = list(self.tracks)
        self.table = np.array(rows, dtype=np.float32)
        return ids, res, np.column_stack([idx1, idx2])

    def _forget(self, tid):
        del self.tracks[tid]
        if tid in self.table_ids:
            i = self.table_ids.index(tid)
            self.table_ids.pop(i)
            self.table = np.delete(self.table, i, axis=0)

    def remove_tracks(self, ids):
        for tid in ids:
            self._forget(int(tid))

    def remove_cameras(self, keys):
        """The feature half of `remove_cameras` (:760-779): views go, tracks without a view go, the rows stay stale."""
        gone = []
        for tid, tr in list(self.tracks.items()):
            keep = [v for v, k in enumerate(tr.keys) if k not in keys]
            for name in ("uv", "desc", "score", "keys"):
                setattr(tr, name, [getattr(tr, name)[v] for v in keep])
            if not tr.keys:
                gone.append(tid)
        for tid in gone:
            self._forget(tid)
        for k in keys:
            self.cams.pop(k, None)
        return gone


class Fixture:
    """`match_frames.npz` by frame: `frame(f)` is a dict of that frame's arrays (prefix f<k>_ stripped)."""

    def __init__(self):
        self.z = np.load(FIXTURE)
        self.n_frames = int(self.z["n_frames"])

    def frame(self, f):
        p = f"f{f}_"
        return {k[len(p):]: self.z[k] for k in self.z.files if k.startswith(p)}

    def tracks(self, fr, stage):
        """{id: (camera keys, lost_for, tracked_for)} after the intake (`stage` "in") or after the frame's removals ("out")."""
        ids, ptr = fr[stage + "_ids"], fr[stage + "_ptr"]
        return {int(t): (fr[stage + "_keys"][ptr[k]:ptr[k + 1]].tolist(), int(fr[stage + "_lost"][k]), int(fr[stage + "_tracked"][k]))
                for k, t in enumerate(ids)}
