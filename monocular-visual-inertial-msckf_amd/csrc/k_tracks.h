// The track store: every floating-point field of the front end's feature tracks resident in HBM, so that a frame sends
// only its new keypoints and a batch is asked for by track id.
//   reference MSCKF.add_camera_measurements (src/msckf/MSCKF.py:403-411, :420-434)  -> k_track_observe
//   the candidate set of MSCKF.get_valid_features / update (:458-495, :570-582)     -> k_track_emit
//   MSCKF.remove_cameras' feature half (:760-779)                                   -> k_track_drop
//   the per-view tests of a frame's matches and the append of those that pass (:332-438) -> k_track_frame
//   the refresh of the inverse-depth point that persists (:484-488)                 -> k_track_writeback
// Rows and positions are decided by the host's integer mirror (msckf_abi.hip) and passed in: no kernel here searches,
// allocates or uses an atomic.  A line's base is the clone's own position array in the reference (:410, :430-431) and an
// inverse-depth point's base that of the clone the track was created in (geometry.py:55): both are resolved from the
// resident clone positions when a batch is emitted, so they follow every injection; an anchor whose clone is removed is
// frozen at the position the clone had then.  fp64 in both dtypes.  All kernels are a few hundred lanes: launch-bound.
#pragma once
#include <hip/hip_runtime.h>

#include "k_assoc.h"
#include "k_select.h"

namespace msckf {

struct TrackStore {
    double* uv;                   // [T][V][2] keypoints
    double* dir;                  // [T][V][3] line directions R_clone K^-1 [u, v, 1], not normalised (Camera.py:30-44)
    double* conf;                 // [T][V]    line confidences (the keypoints' scores)
    int* slot;                    // [T][V]    clone slot of each view, ascending
    double* m;                    // [T][3]    InverseDepthPoint.m
    double* rho;                  // [T]       InverseDepthPoint.rho
    double* frozen;               // [T][3]    the anchor clone's last position, once it was removed
    int* anchor;                  // [T]       slot of the clone the track was created in; -1: frozen
    int* count;                   // [T]       views
    int V;                        // views a row holds (the context's max_track)
};

struct __attribute__((aligned(8))) TrackObsRec {
    int row, pos;                 // where the view goes
    int fresh, pad;               // 1: the track is created by this view
    double u, v, score;
};

struct TrackObsArgs {
    TrackStore s;
    const TrackObsRec* rec;       // [n] (pinned host image)
    int n, slot;                  // slot: the newest clone's, N - 1
    const double* R;              // its rotation (3 x 3, resident)
    double Kinv[9];
};

// The store of one new view (shared by k_track_observe and k_track_frame: the stored bits are the same whoever appends).
__device__ __forceinline__ void track_store_view(const TrackStore& s, const TrackObsRec& r, int slot, const double* R, const double* Kinv) {
    const double ex = Kinv[0] * r.u + Kinv[1] * r.v + Kinv[2];            // Camera.inverse_project_point (Camera.py:30-36)
    const double ey = Kinv[3] * r.u + Kinv[4] * r.v + Kinv[5];
    const double ez = Kinv[6] * r.u + Kinv[7] * r.v + Kinv[8];
    const double gx = R[0] * ex + R[1] * ey + R[2] * ez;                  // Ci2W, rotation only (:38-44)
    const double gy = R[3] * ex + R[4] * ey + R[5] * ez;
    const double gz = R[6] * ex + R[7] * ey + R[8] * ez;
    const size_t e = (size_t)r.row * s.V + r.pos;
    s.uv[2 * e] = r.u; s.uv[2 * e + 1] = r.v;
    s.dir[3 * e] = gx; s.dir[3 * e + 1] = gy; s.dir[3 * e + 2] = gz;
    s.conf[e] = r.score;
    s.slot[e] = slot;
    s.count[r.row] = r.pos + 1;
    if (r.fresh) {                                                        // InverseDepthPoint(camera pose, W_v), geometry.py:53-59
        const double gn = sqrt(gx * gx + gy * gy + gz * gz);
        s.m[3 * (size_t)r.row] = gx / gn; s.m[3 * (size_t)r.row + 1] = gy / gn; s.m[3 * (size_t)r.row + 2] = gz / gn;
        s.rho[r.row] = 0.1;
        s.anchor[r.row] = slot;
    }
}

// One lane per new view.
__global__ __launch_bounds__(256) void k_track_observe(TrackObsArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const TrackObsRec r = p.rec[i];
    track_store_view(p.s, r, p.slot, p.R, p.Kinv);
}

struct __attribute__((aligned(8))) TrackEmitRec {
    int row, M;                   // the candidate's row and views
    int a, o;                     // its first view in the batch's input order / in the sorted order
    int sidx;                     // its sorted position
    int lost, tracked;            // the front end's counters (they live on the host)
    int pad;
};

struct TrackEmitArgs {
    TrackStore s;
    const TrackEmitRec* rec;      // [F] input order (pinned host image)
    int F;
    const double* cam_t;          // [N][3] resident clone positions
    // the batch's raw image, input order: what k_gather reads
    double* uv_raw; int* slot_raw; double* base_raw; double* m_raw; double* rho_raw;
    // what k_select reads, sorted order
    double* line_base; double* line_dir; double* line_conf; int* lost_for; int* tracked_for;
    int* row_sorted;              // [F] sorted position -> row (k_track_writeback)
};

constexpr int TRACK_THREADS = 256;

// The per-row kernels give a row a group of G lanes, lane v carrying view v.  G = 32: two rows share a wavefront, each takes
// its half of the wavefront's ballot as a 32-bit mask (the store of a context with max_track <= 32).  G = 64: a wavefront
// per row, the whole 64-bit ballot is the row's (a context created with MSCKF_FLAG_WIDE_STORE, rows of up to 64 views).
template <int G> struct TrackGroup;
template <> struct TrackGroup<32> {
    using mask_t = unsigned;
    static __device__ __forceinline__ mask_t mine(unsigned long long b) { return (unsigned)(b >> (threadIdx.x & 32)); }
    static __device__ __forceinline__ mask_t below(int v) { return (1u << v) - 1u; }
    static __device__ __forceinline__ int popc(mask_t m) { return __popc(m); }
    static __device__ __forceinline__ int ffs(mask_t m) { return __ffs(m); }
};
template <> struct TrackGroup<64> {
    using mask_t = unsigned long long;
    static __device__ __forceinline__ mask_t mine(unsigned long long b) { return b; }
    static __device__ __forceinline__ mask_t below(int v) { return (1ull << v) - 1ull; }
    static __device__ __forceinline__ int popc(mask_t m) { return __popcll(m); }
    static __device__ __forceinline__ int ffs(mask_t m) { return __ffsll(m); }
};
constexpr int track_group_log2(int G) { return G == 64 ? 6 : 5; }

// One G-lane group per candidate; lane v carries view v (v < M <= V <= G).
template <int G>
__global__ __launch_bounds__(TRACK_THREADS) void k_track_emit(TrackEmitArgs p) {
    static_assert(G == 32 || G == 64, "a row's group is half a wavefront or a whole one");
    const int v = threadIdx.x & (G - 1);
    const int f = blockIdx.x * (TRACK_THREADS / G) + (threadIdx.x >> track_group_log2(G));
    if (f >= p.F) return;
    const TrackEmitRec r = p.rec[f];
    const size_t row = (size_t)r.row;
    if (v < r.M) {
        const size_t e = row * p.s.V + v;
        const int sl = p.s.slot[e];
        const size_t in = (size_t)r.a + v, out = (size_t)r.o + v;
        p.uv_raw[2 * in] = p.s.uv[2 * e]; p.uv_raw[2 * in + 1] = p.s.uv[2 * e + 1];
        p.slot_raw[in] = sl;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p.line_base[3 * out + k] = p.cam_t[3 * (size_t)sl + k];       // Line.base IS the clone's position (MSCKF.py:410)
            p.line_dir[3 * out + k] = p.s.dir[3 * e + k];
        }
        p.line_conf[out] = p.s.conf[e];
    }
    // (the head of the track on lanes that are free in the shortest track as well as busy in the longest; in a row of 64 views
    //  every lane carries a view, these eight among them)
    if (v < 3) {
        const int an = p.s.anchor[row];
        p.base_raw[3 * (size_t)f + v] = an >= 0 ? p.cam_t[3 * (size_t)an + v] : p.s.frozen[3 * row + v];
    } else if (v < 6) {
        p.m_raw[3 * (size_t)f + v - 3] = p.s.m[3 * row + v - 3];
    } else if (v == 6) {
        p.rho_raw[f] = p.s.rho[row];
    } else if (v == 7) {
        p.lost_for[r.sidx] = r.lost; p.tracked_for[r.sidx] = r.tracked; p.row_sorted[r.sidx] = r.row;
    }
}

struct TrackDropArgs {
    TrackStore s;
    const int* rows;              // [n] the rows that hold a track
    int n;
    const double* cam_t;          // clone positions as they stand BEFORE the removal
    short remap[224];             // old slot -> new slot, -1: removed (a window holds at most 221 clones)
};

// One G-lane group per track: drop the views of removed clones, close the gaps, renumber, freeze the anchor.
template <int G>
__global__ __launch_bounds__(TRACK_THREADS) void k_track_drop(TrackDropArgs p) {
    static_assert(G == 32 || G == 64, "a row's group is half a wavefront or a whole one");
    using Grp = TrackGroup<G>;
    const int v = threadIdx.x & (G - 1);
    const int g = blockIdx.x * (TRACK_THREADS / G) + (threadIdx.x >> track_group_log2(G));
    const bool live = g < p.n;
    const size_t row = live ? (size_t)p.rows[g] : 0;
    const int M = live ? p.s.count[row] : 0;
    const size_t e = row * p.s.V + v;
    bool keep = false;
    int ns = -1;
    double u0 = 0, u1 = 0, d0 = 0, d1 = 0, d2 = 0, cf = 0;
    if (v < M) {
        ns = p.remap[p.s.slot[e]];
        keep = ns >= 0;
        u0 = p.s.uv[2 * e]; u1 = p.s.uv[2 * e + 1];
        d0 = p.s.dir[3 * e]; d1 = p.s.dir[3 * e + 1]; d2 = p.s.dir[3 * e + 2];
        cf = p.s.conf[e];
    }
    // the group's share of the wavefront's ballot (G = 32: its half; G = 64: all of it); a view moves down by the number of
    // dropped views in front of it.  (Every lane of the wavefront has read its view by now: the stores below wait for the
    // loads above.)
    const unsigned long long b = __ballot(keep);
    const typename Grp::mask_t mine = Grp::mine(b);
    if (keep) {
        const size_t w = row * p.s.V + Grp::popc(mine & Grp::below(v));
        p.s.uv[2 * w] = u0; p.s.uv[2 * w + 1] = u1;
        p.s.dir[3 * w] = d0; p.s.dir[3 * w + 1] = d1; p.s.dir[3 * w + 2] = d2;
        p.s.conf[w] = cf;
        p.s.slot[w] = ns;
    }
    if (live && v == 0) {
        p.s.count[row] = Grp::popc(mine);
        const int an = p.s.anchor[row];
        if (an >= 0) {
            const int na = p.remap[an];
            if (na < 0) {                                                 // the base keeps the clone's last position
                p.s.frozen[3 * row] = p.cam_t[3 * (size_t)an]; p.s.frozen[3 * row + 1] = p.cam_t[3 * (size_t)an + 1];
                p.s.frozen[3 * row + 2] = p.cam_t[3 * (size_t)an + 2];
            }
            p.s.anchor[row] = na;
        }
    }
}

// A frame's matches on the store (reference MSCKF.add_camera_measurements, :332-438): the association test of k_assoc.h of
// every listed (track, keypoint) pair against the track's stored views, with the newest clone's pose read where it is
// resident, and the append of the pairs that pass.
struct TrackFrameArgs {
    TrackStore s;
    const TrackObsRec* rec;       // [n] (pinned host image); pos = the row's view count, the position an append takes
    int n, slot;                  // slot: the newest clone's, N - 1
    const double* cam_R;          // [N][9], [N][3] resident clone poses
    const double* cam_t;
    double K[9], Kinv_test[9];    // the intrinsics and their inverse as the tests form it (MSCKF.py:345)
    double Kinv[9];               // the context's K^-1: the stored direction
    double thr_epipolar, thr_homography;
    int* fail_view;               // [n] (pinned host memory) first view that failed, -1
    unsigned char* result;        // [n] (pinned host memory) 0 appended, 1 epipolar failure, 2 homography failure, 4 created
};

// One G-lane group per pair; lane v tests stored view v (a tested row holds at most G - 1: the mirror refuses a full row).
// The group's share of the wavefront's ballot gives the first failing view, where the reference breaks (:369, :390).  Lane
// 0 appends: position `pos` (<= V - 1) is read by no lane (v < pos), and every pair has a row of its own.  Every lane
// reaches both ballots: the early exit stands behind them.
template <int G>
__global__ __launch_bounds__(TRACK_THREADS) void k_track_frame(TrackFrameArgs p) {
    static_assert(G == 32 || G == 64, "a row's group is half a wavefront or a whole one");
    using Grp = TrackGroup<G>;
    const int v = threadIdx.x & (G - 1);
    const int g = blockIdx.x * (TRACK_THREADS / G) + (threadIdx.x >> track_group_log2(G));
    const bool live = g < p.n;
    TrackObsRec r{};
    if (live) r = p.rec[g];
    const int M = (live && !r.fresh) ? r.pos : 0;
    const double* R2 = p.cam_R + 9 * (size_t)p.slot;
    const double* t2 = p.cam_t + 3 * (size_t)p.slot;
    int code = 0;
    if (v < M) {
        const size_t e = (size_t)r.row * p.s.V + v;
        const int sl = p.s.slot[e];
        code = assoc_view_test(p.K, p.Kinv_test, p.cam_R + 9 * (size_t)sl, p.cam_t + 3 * (size_t)sl, R2, t2, p.s.uv[2 * e], p.s.uv[2 * e + 1],
                               r.u, r.v, p.thr_epipolar, p.thr_homography);
    }
    const unsigned long long bf = __ballot(code != 0), bh = __ballot(code == 2);
    const typename Grp::mask_t fails = Grp::mine(bf), homs = Grp::mine(bh);
    if (!live || v != 0) return;
    const int first = fails ? Grp::ffs(fails) - 1 : -1;
    p.fail_view[g] = first;
    p.result[g] = r.fresh ? 4 : first < 0 ? 0 : ((homs >> first) & 1u) ? 2 : 1;
    if (first < 0) track_store_view(p.s, r, p.slot, R2, p.Kinv);
}

// Behind k_select: the refreshed inverse-depth points go back to their rows (the reference's refresh persists).
__global__ __launch_bounds__(256) void k_track_writeback(TrackStore s, int F, const unsigned char* __restrict__ flags,
                                                         const double* __restrict__ idp_m, const double* __restrict__ idp_rho,
                                                         const int* __restrict__ row_sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F || !(flags[i] & SEL_REFRESHED)) return;
    const size_t row = (size_t)row_sorted[i];
    s.m[3 * row] = idp_m[3 * (size_t)i]; s.m[3 * row + 1] = idp_m[3 * (size_t)i + 1]; s.m[3 * row + 2] = idp_m[3 * (size_t)i + 2];
    s.rho[row] = idp_rho[i];
}

}  // namespace msckf
