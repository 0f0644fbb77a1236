"""Loader of the 30-clone filter run `golden/window30/seq_window30.npz` (written by `golden/gen_golden.py --window30`).

The run is the reference's `feature_callback` order (`MSCKF.py:147-158`) over ~40 frames: per frame four IMU samples,
one augmentation, one `process_features` (selection, update, `remove_features`, whose tail may drop clones that no
feature sees any more) and, above 30 clones, `prune_poorest_camera_states`.  Ops, in order (`op_kind`):
0 IMU sample, 1 augmentation, 2 process_features' selection + update, 3 prune (selection + update + removal of its two
clones), 4 removal of the clones `remove_features` left without features.  Each selection the reference ran is a
"call" (kinds 2 and 3), stored flat with offsets; its views point into one global observation pool.

The lines' and inverse-depth points' bases are what the reference held at the call's entry.  The reference builds both
on the clone's own position array (`MSCKF.py:410, :430-431`), so they move with every injection; an inverse-depth
point whose anchor clone was pruned keeps that clone's last position.  Stored deduplicated per call (`call_bases`
and indices into it).  Not a conftest: imported by name."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "window30", "seq_window30.npz")
SIZE_LIMIT = 1 << 20                     # bytes: a committed file stays within 1 MiB (seq_long.npz, the largest fixture before, is 1.75 MB)

IMU, AUGMENT, PROCESS, PRUNE, REMOVE = 0, 1, 2, 3, 4
SPLIT_SPAN = 15                         # tracks over more clone slots than this are split
MIN_MARGIN = 1e-6


def _span(p, i):
    return slice(int(p[i]), int(p[i + 1]))


class Run:
    def __init__(self, z=None):
        if z is None:
            z = np.load(PATH)
        self.z = {k: z[k] for k in (z.files if hasattr(z, "files") else z.keys())}
        z = self.z
        self.ops = list(zip(z["op_kind"].tolist(), z["op_index"].tolist()))
        self.probes = {}
        # probes are stacked in op order; their sizes follow from the clone count after each op
        sizes = self._dims()
        off = 0
        for o in z["probe_op"]:
            d = sizes[int(o)]
            self.probes[int(o)] = z["probe"][off:off + d]
            off += d
        assert off == z["probe"].shape[0]
        self.checkpoints = {}
        off = 0
        for o in z["ckpt_op"]:
            d = sizes[int(o)]
            t = d * (d + 1) // 2
            P = np.zeros((d, d))
            iu = np.triu_indices(d)
            P[iu] = z["ckpt"][off:off + t]
            P.T[iu] = z["ckpt"][off:off + t]
            self.checkpoints[int(o)] = P
            off += t
        assert off == z["ckpt"].shape[0]
        # inverse-depth points at entry: stored only where they changed since the feature's previous call
        self._m, self._rho = np.zeros((len(z["call_ids"]), 3)), np.zeros(len(z["call_ids"]))
        last, r = {}, 0
        for row, (fid, chg) in enumerate(zip(z["call_ids"].tolist(), z["call_mchg"])):
            if chg:
                last[fid] = (z["call_m"][r], z["call_rho"][r])
                r += 1
            self._m[row], self._rho[row] = last[fid]
        assert r == len(z["call_rho"])
        self.K = z["K"]
        self.sigma = float(z["sigma"])
        self.gravity = z["gravity"]
        self.V = z["V"]

    def _dims(self):
        """Covariance size after every op."""
        N, out = 0, []
        for kind, idx in self.ops:
            if kind == AUGMENT:
                N += 1
            elif kind in (PRUNE, REMOVE):
                N -= int(self.z["call_rmptr"][idx + 1] - self.z["call_rmptr"][idx])
            out.append(15 + 6 * N)
        return out

    def n_clones_after(self):
        return [(d - 15) // 6 for d in self._dims()]

    def imu(self, i):
        z = self.z
        return {k: z["imu_" + k][i] for k in ("acc", "gyro", "dt", "R", "t", "v", "R0", "t0", "v0", "w_planet")}

    def aug(self, i):
        z = self.z
        return {k: z["aug_" + k][i] for k in ("imu_R", "imu_t", "cam_R", "cam_t", "key")}

    def n_calls(self):
        return len(self.z["call_kind"])

    def call(self, i):
        """Everything one selection call read and what the reference did with it; per-view arrays in the call's CSR."""
        z = self.z
        fs, vs, bs = _span(z["call_fptr"], i), _span(z["call_vptr"], i), _span(z["call_bptr"], i)
        keys = z["call_keys"][_span(z["call_kptr"], i)]
        slot_of = {int(k): s for s, k in enumerate(keys)}
        pool = z["call_pool"][vs]
        bases = z["call_bases"][bs]
        nview = z["call_nview"][fs].astype(np.int64)
        F = len(nview)
        flags = z["call_flags"][fs]
        m, rho = self._m[fs].copy(), self._rho[fs].copy()
        ref = np.nonzero(flags & 4)[0]
        rs = _span(z["call_rptr"], i)
        sel_m, sel_rho = m.copy(), rho.copy()
        sel_m[ref], sel_rho[ref] = z["call_ref_m"][rs], z["call_ref_rho"][rs]
        world = np.full((F, 3), np.nan)
        world[ref] = z["call_ref_world"][rs]
        return dict(
            kind=int(z["call_kind"][i]), frame=int(z["call_frame"][i]), keys=keys, ids=z["call_ids"][fs],
            lost=z["call_lost"][fs].astype(np.int32), tracked=z["call_tracked"][fs].astype(np.int32),
            view_ptr=np.concatenate([[0], np.cumsum(nview)]).astype(np.int32), pool=pool,
            obs_uv=z["pool_uv"][pool].astype(np.float64), obs_slot=np.array([slot_of[int(k)] for k in z["pool_key"][pool]], dtype=np.int32),
            obs_key=z["pool_key"][pool], obs_lid=z["pool_lid"][pool],
            line_base=bases[z["call_vbase"][vs]], line_dir=z["pool_dir"][pool], line_conf=z["pool_score"][pool].astype(np.float64),
            idp_base=bases[z["call_ibase"][fs]], idp_m=m, idp_rho=rho,
            flags=flags, sel_m=sel_m, sel_rho=sel_rho, world=world, accepted=z["call_accepted"][fs],
            status=int(z["call_status"][i]), n_rejected=int(z["call_n_rejected"][i]), qr=int(z["call_qr"][i]),
            dx=z["call_dx"][_span(z["call_dxptr"], i)], rm=z["call_rm"][_span(z["call_rmptr"], i)],
            post_R=z["call_post_R"][_span(z["call_pptr"], i)], post_t=z["call_post_t"][_span(z["call_pptr"], i)],
            counts=z["call_counts"][_span(z["call_cptr"], i)],
            exit_ids=z["call_exit_ids"][_span(z["call_eptr"], i)], exit_nview=z["call_exit_nview"][_span(z["call_eptr"], i)])

    def select_params(self):
        from msckf_amd import synth
        sp = self.z["select_params"]
        return synth.SelectParams(min_frames_lost=int(sp[0]), min_frames_tracked=int(sp[1]), use_parallax=bool(sp[2]),
                                  min_parallax_deg=float(sp[3]), width=int(sp[4]), height=int(sp[5]))

    def problem(self, c, P, cam_R, cam_t):
        """The call's batch as the engine takes it; null poses = current poses (Camera.py:10-11)."""
        from msckf_amd import synth
        return synth.UpdateProblem(P=P, cam_R=cam_R, cam_t=cam_t, cam_R0=cam_R, cam_t0=cam_t, gravity=self.gravity,
                                   K=self.K, sigma=self.sigma, view_ptr=c["view_ptr"], obs_uv=c["obs_uv"],
                                   obs_slot=c["obs_slot"], idp_base=c["idp_base"], idp_m=c["idp_m"].copy(),
                                   idp_rho=c["idp_rho"].copy())

    @staticmethod
    def tracks(c):
        from msckf_amd import synth
        return synth.TrackTable(line_base=c["line_base"], line_dir=c["line_dir"], line_conf=c["line_conf"],
                                lost_for=c["lost"], tracked_for=c["tracked"])


def poorest_two(counts):
    """`prune_poorest_camera_states`' choice (`MSCKF.py:712-724`): the first two clone keys of a stable sort of the
    (key, count) pairs, which are in the order the reference's dictionary met them."""
    return [int(k) for k, _ in sorted(counts.tolist(), key=lambda kv: kv[1])[:2]]


def properties(run):
    """The run's coverage, from the stored arrays alone."""
    z = run.z
    aug_keys = [int(k) for k in z["aug_key"]]
    frame_of_key = {k: i for i, k in enumerate(aug_keys)}
    split_updates, long_accepted, holes, branches = 0, 0, 0, set()
    n_prune, n_remove, prune_updates, middle_prunes, pruned_inside, pruned_keys = 0, 0, 0, 0, 0, []
    for i in range(run.n_calls()):
        c = run.call(i)
        vp = c["view_ptr"]
        valid = np.nonzero(c["flags"] & 1)[0]
        if c["kind"] == PRUNE:
            n_prune += 1
            prune_updates += int(c["status"] == 0)
        elif len(c["rm"]):
            n_remove += 1
        if c["status"] == 0:
            branches.add(c["qr"])
            spans = [int(c["obs_slot"][vp[j + 1] - 1] - c["obs_slot"][vp[j]] + 1) for j in valid]
            if max(spans) > SPLIT_SPAN:
                split_updates += 1
        if c["kind"] == PRUNE and sorted(c["rm"].tolist()) != [0, 1]:
            middle_prunes += 1
        pruned = set(pruned_keys)
        for j in np.nonzero(c["accepted"])[0]:
            n = int(vp[j + 1] - vp[j])
            long_accepted = max(long_accepted, n)
            slots = c["obs_slot"][vp[j]:vp[j + 1]]
            if n > 10 and slots[-1] - slots[0] + 1 > n:
                holes += 1                  # views skip a clone of the window
            frames = [frame_of_key[int(k)] for k in c["obs_key"][vp[j]:vp[j + 1]]]
            if n > 10 and any(aug_keys[fr] in pruned for fr in range(frames[0], frames[-1] + 1)):
                pruned_inside += 1          # ... and a pruned clone lay inside the span of views it kept
        if c["kind"] == PRUNE:
            pruned_keys.extend(int(c["keys"][s]) for s in c["rm"])
    stale = 0
    for i in range(run.n_calls()):
        c = run.call(i)
        live = {tuple(b) for b in c["line_base"]}
        stale += int(sum(tuple(b) not in live for b in c["idp_base"][(c["flags"] & 1) > 0]))
    return dict(max_clones=max(run.n_clones_after()), prunes=n_prune, prune_updates=prune_updates, feature_removals=n_remove,
                split_updates=split_updates, longest_accepted=long_accepted, long_tracks_with_holes=holes,
                prunes_not_oldest=middle_prunes, long_tracks_over_pruned_clones=pruned_inside,
                update_branches=sorted(branches), stale_anchor_selections=stale, margins=z["margins"].tolist(),
                calls=run.n_calls(), pool=int(len(z["pool_uv"])))


def assert_properties(p):
    assert p["max_clones"] == 31, p
    assert p["prunes"] >= 8 and p["prune_updates"] >= 1, p
    assert p["split_updates"] >= 10, p
    assert p["longest_accepted"] >= 25, p
    assert p["long_tracks_with_holes"] > 0 and p["prunes_not_oldest"] > 0 and p["long_tracks_over_pruned_clones"] > 0, p
    assert p["update_branches"] == [0, 1], p
    assert min(p["margins"]) > MIN_MARGIN, p
