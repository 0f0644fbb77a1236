// Descriptor matching on the track store: the front end's mutual-nearest-neighbour match (reference
// FeatureExtractor.match, src/msckf/FeatureExtractor.py:62-84, around XFeat.match) against the table the reference keeps as
// last_camera_measurement (MSCKF.py:436-444), and the per-view descriptors behind that table.
//   S = A B^T, m12 = argmax_j, m21 = argmax_i, mutual and S > min_cosine_similarity (strict)   -> k_match_argmax (twice), k_match_resolve
//   feature.descriptors.append (MSCKF.py:302, :407, :427)                                        -> k_desc_store
//   np.average(feature.descriptors, axis=0, weights=feature.scores) (:439), raw rows (:311)     -> k_desc_average
//   del feature.descriptors[camera_index] (:766)                                                 -> k_desc_drop
//   the same match behind a search window and a distinctiveness margin (not in the reference)   -> k_match_last_uv,
//                                                                     k_match_argmax_opt (twice), k_match_resolve_opt
// A is the table, one fp32 row of 64 per track ([T][64] by device row, rows shorter than 64 are zero-padded), visited in the
// order the tracks were created through the row list the host's mirror hands in; B is the frame, [n][64].  S is never
// stored: a wavefront owns 16 rows of one operand, walks the other operand in tiles of 16 with 16 chained
// v_mfma_f32_16x16x4_f32 per tile and keeps a running (max, lowest index) per accumulator register.  Ties go to the lowest
// index: tiles ascend and only a strictly larger value replaces the running one; the closing reduction over the 16 lanes of
// a DPP row prefers the lower index of equal values.  No atomics, no waits between workgroups, no searches.
#pragma once
#include <hip/hip_runtime.h>

#include "k_tracks.h"

namespace msckf {

constexpr int DESC_DIM = 64;      // floats a stored descriptor row holds (XFeat's dimension; shorter ones are zero-padded)

struct DescStore {
    float* views;                 // [T][V][64] per-view descriptors
    float* row;                   // [T][64]    the match row of each track (a snapshot: recomputed at the end of an intake only)
    int V;
};

struct MatchArgmaxArgs {
    const float* X; const int* xrows; int nx;     // the operand whose rows are answered; xrows: element -> row of X, null: identity
    const float* Y; const int* yrows; int ny;     // the operand that is searched
    int* best;                                    // [nx] argmax over Y's elements, lowest index among equals
    float* sim;                                   // [nx] the maximum (nullable)
};

typedef float match_v4f __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ void match_fold(float& v, int& j) {
    const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
    const int oj = __builtin_amdgcn_update_dpp(0, j, CTRL, 0xf, 0xf, false);
    if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; }
}

// One wavefront per 16 elements of X.  Operand maps of v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][k = l >> 4] and
// B[k = l >> 4][l & 15]; C/D: col = l & 15, row = 4 (l >> 4) + reg (k_gain.h).  The sum over the 64 dimensions does not
// care which four of them a step takes, so lane group g = l >> 4 takes dimensions 16 g .. 16 g + 15, one per step: a
// lane's share of a descriptor is 16 consecutive floats, four 16-byte loads.
__global__ __launch_bounds__(64) void k_match_argmax(MatchArgmaxArgs p) {
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.x * 16;
    float4 a[4] = {};
    if (i0 + r < p.nx) {
        const size_t row = p.xrows ? (size_t)p.xrows[i0 + r] : (size_t)(i0 + r);
        const float4* src = reinterpret_cast<const float4*>(p.X + row * DESC_DIM + 16 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = src[q];
    }
    float bv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bj[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    for (int j0 = 0; j0 < p.ny; j0 += 16) {
        const int j = j0 + r;
        float4 b[4] = {};
        if (j < p.ny) {
            const size_t row = p.yrows ? (size_t)p.yrows[j] : (size_t)j;
            const float4* src = reinterpret_cast<const float4*>(p.Y + row * DESC_DIM + 16 * g);
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = src[q];
        }
        match_v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].x, b[q].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].y, b[q].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].z, b[q].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].w, b[q].w, acc, 0, 0, 0);
        }
        if (j < p.ny) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (acc[q] > bv[q] || bj[q] == 0x7fffffff) { bv[q] = acc[q]; bj[q] = j; }
        }
    }
    // register q of lane group g is element i0 + 4 g + q; its 16 columns are the 16 lanes of the DPP row
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        match_fold<0xB1>(bv[q], bj[q]);       // quad_perm [1,0,3,2]: lane ^ 1
        match_fold<0x4E>(bv[q], bj[q]);       // quad_perm [2,3,0,1]: lane ^ 2
        match_fold<0x141>(bv[q], bj[q]);      // row_half_mirror: the two quads of each 8
        match_fold<0x140>(bv[q], bj[q]);      // row_mirror: the two halves of the row
    }
    if (r < 4) {                              // lane r of the row writes register r (a select chain: no indexed registers)
        const float v = r == 0 ? bv[0] : r == 1 ? bv[1] : r == 2 ? bv[2] : bv[3];
        const int j = r == 0 ? bj[0] : r == 1 ? bj[1] : r == 2 ? bj[2] : bj[3];
        const int i = i0 + 4 * g + r;
        if (i < p.nx) {
            p.best[i] = j;
            if (p.sim) p.sim[i] = v;
        }
    }
}

// One lane per table element i: (i, m12[i]) is a pair iff m21[m12[i]] == i and S > min_cos.  pair[T] and sim[T] are pinned
// host memory (the mirror turns them into track ids); plain vector stores.
__global__ __launch_bounds__(256) void k_match_resolve(int T, const int* __restrict__ m12, const float* __restrict__ sim12,
                                                       const int* __restrict__ m21, double min_cos, int* pair, float* sim) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const int j = m12[i];
    const float s = sim12[i];
    pair[i] = (m21[j] == i && (double)s > min_cos) ? j : -1;
    sim[i] = s;
}

// ---- the match with a search window and a distinctiveness margin (NOT in the reference) -------------------------
// allowed(i, j): the window is off, or (u_j - u^_i)^2 + (v_j - v^_i)^2 <= radius^2 in double, (u^_i, v^_i) the last stored
// keypoint of table track i.  S'[i][j] = S[i][j] where allowed, else -inf; per element of the answered operand the kernel
// keeps (best, lowest index of the best, second best) of S'; "none allowed" is index -1 with best = second = -inf.

// The table's last keypoints as a dense [T][2] array in creation order: view count - 1 of each listed row as the store
// holds it now (behind an append the appended keypoint, behind k_track_drop the last view that survived).  One lane per track.
__global__ __launch_bounds__(256) void k_match_last_uv(TrackStore s, const int* __restrict__ rows, int T, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const size_t row = (size_t)rows[t];
    const int last = s.count[row] - 1;                // (a live track holds a view; the clamp keeps a stale count inside the row)
    const size_t e = row * s.V + (last < 0 ? 0 : last >= s.V ? s.V - 1 : last);
    out[2 * (size_t)t] = s.uv[2 * e];
    out[2 * (size_t)t + 1] = s.uv[2 * e + 1];
}

struct MatchOptArgs {
    const float* X; const int* xrows; int nx;     // as MatchArgmaxArgs
    const float* Y; const int* yrows; int ny;
    const double* xuv; const double* yuv;         // [nx][2], [ny][2] keypoints by ELEMENT (not by row); unread when window == 0
    double r2;                                    // radius^2 (+inf is legal)
    int window;                                   // 0: every (i, j) is allowed
    int* best;                                    // [nx] argmax of S', lowest index among equals; -1: none allowed
    float* s1;                                    // [nx] that maximum (-inf: none)
    float* s2;                                    // [nx] the largest S' over the other elements (-inf: none)
};

// Merge the triple of the lane CTRL names into this lane's: the best by (value, then lower index), the second the
// maximum of the loser's best and both seconds.
template <int CTRL>
__device__ __forceinline__ void match_fold3(float& v, int& j, float& s) {
    const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
    const int oj = __builtin_amdgcn_update_dpp(0, j, CTRL, 0xf, 0xf, false);
    const float os = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), CTRL, 0xf, 0xf, false));
    const bool other = ov > v || (ov == v && oj < j);
    const float loser = other ? v : ov;
    if (other) { v = ov; j = oj; }
    s = fmaxf(loser, fmaxf(s, os));
}

// k_match_argmax's shape (one wavefront per 16 elements of X, Y walked in tiles of 16, 16 chained MFMA per tile, the same
// operand maps, so S has the bits k_match_argmax forms); new: the mask behind the chain and the second best.  Register q
// of lane (r, g) is S[i0 + 4 g + q][j0 + r]: the lane keeps the keypoints of its four rows and loads its column's per tile.
__global__ __launch_bounds__(64) void k_match_argmax_opt(MatchOptArgs p) {
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.x * 16;
    float4 a[4] = {};
    if (i0 + r < p.nx) {
        const size_t row = p.xrows ? (size_t)p.xrows[i0 + r] : (size_t)(i0 + r);
        const float4* src = reinterpret_cast<const float4*>(p.X + row * DESC_DIM + 16 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = src[q];
    }
    double xu[4] = {0.0, 0.0, 0.0, 0.0}, xv[4] = {0.0, 0.0, 0.0, 0.0};
    if (p.window) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + 4 * g + q;
            if (i < p.nx) { xu[q] = p.xuv[2 * (size_t)i]; xv[q] = p.xuv[2 * (size_t)i + 1]; }
        }
    }
    float bv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    float sv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bj[4] = {-1, -1, -1, -1};
    for (int j0 = 0; j0 < p.ny; j0 += 16) {
        const int j = j0 + r;
        float4 b[4] = {};
        double yu = 0.0, yv = 0.0;
        if (j < p.ny) {
            const size_t row = p.yrows ? (size_t)p.yrows[j] : (size_t)j;
            const float4* src = reinterpret_cast<const float4*>(p.Y + row * DESC_DIM + 16 * g);
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = src[q];
            if (p.window) { yu = p.yuv[2 * (size_t)j]; yv = p.yuv[2 * (size_t)j + 1]; }
        }
        match_v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].x, b[q].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].y, b[q].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].z, b[q].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].w, b[q].w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bool ok = j < p.ny;
            if (p.window) {                       // products and sum rounded one by one, as NumPy rounds them
                const double du = yu - xu[q], dv = yv - xv[q];
                ok = ok && __dadd_rn(__dmul_rn(du, du), __dmul_rn(dv, dv)) <= p.r2;
            }
            const float v = ok ? acc[q] : -INFINITY;
            if (v > bv[q]) { sv[q] = bv[q]; bv[q] = v; bj[q] = j; }
            else if (v > sv[q]) sv[q] = v;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        match_fold3<0xB1>(bv[q], bj[q], sv[q]);      // the four folds of k_match_argmax
        match_fold3<0x4E>(bv[q], bj[q], sv[q]);
        match_fold3<0x141>(bv[q], bj[q], sv[q]);
        match_fold3<0x140>(bv[q], bj[q], sv[q]);
    }
    if (r < 4) {
        const float v = r == 0 ? bv[0] : r == 1 ? bv[1] : r == 2 ? bv[2] : bv[3];
        const float s = r == 0 ? sv[0] : r == 1 ? sv[1] : r == 2 ? sv[2] : sv[3];
        const int j = r == 0 ? bj[0] : r == 1 ? bj[1] : r == 2 ? bj[2] : bj[3];
        const int i = i0 + 4 * g + r;
        if (i < p.nx) { p.best[i] = j; p.s1[i] = v; p.s2[i] = s; }
    }
}

// One lane per table element i: its reason code, the first that applies -- 1 no keypoint inside the window, 2 not mutual,
// 3 not s1 > min_cos, 4 (margin > 0) not (s1 - s2 > margin and c1 - c2 > margin), 0 the pair (i, m12[i]); every comparison
// strict and in double on the fp32 values, a second best of -inf passes.  pair[T], sim[T], why[T] are pinned host memory.
__global__ __launch_bounds__(256) void k_match_resolve_opt(int T, const int* __restrict__ m12, const float* __restrict__ s1,
                                                           const float* __restrict__ s2, const int* __restrict__ m21,
                                                           const float* __restrict__ c1, const float* __restrict__ c2,
                                                           double min_cos, double margin, int* pair, float* sim, int* why) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const int j = m12[i];
    const float s = s1[i];
    int code = 0;
    if (j < 0) code = 1;
    else if (m21[j] != i) code = 2;
    else if (!((double)s > min_cos)) code = 3;
    else if (margin > 0.0 && !((double)s - (double)s2[i] > margin && (double)c1[j] - (double)c2[j] > margin)) code = 4;
    pair[i] = code == 0 ? j : -1;
    sim[i] = s;
    why[i] = code;
}

struct __attribute__((aligned(8))) DescRec { int row, pos, j, pad; };   // view `pos` of track `row` gets the frame's descriptor j

// One 64-lane wavefront per record, lane = dimension.
__global__ __launch_bounds__(64) void k_desc_store(DescStore s, const DescRec* __restrict__ rec, const float* __restrict__ frame) {
    const DescRec r = rec[blockIdx.x];
    s.views[((size_t)r.row * s.V + r.pos) * DESC_DIM + threadIdx.x] = frame[(size_t)r.j * DESC_DIM + threadIdx.x];
}

// One 64-lane wavefront per track, lane = dimension: row = fp32(sum_v fp64(d_v) conf_v / sum_v conf_v) over the track's
// views in view order, products and sums rounded one by one as NumPy rounds them; raw: the first view's bits (:311).
__global__ __launch_bounds__(64) void k_desc_average(DescStore s, TrackStore t, const int* __restrict__ rows, int raw) {
    const size_t row = (size_t)rows[blockIdx.x];
    const int d = threadIdx.x;
    const float* v = s.views + row * s.V * DESC_DIM + d;
    if (raw) { s.row[row * DESC_DIM + d] = v[0]; return; }
    const int M = t.count[row];
    double num = 0.0, den = 0.0;
    for (int k = 0; k < M; ++k) {
        const double w = t.conf[row * t.V + k];
        num = __dadd_rn(num, __dmul_rn((double)v[(size_t)k * DESC_DIM], w));
        den = __dadd_rn(den, w);
    }
    s.row[row * DESC_DIM + d] = (float)(num / den);
}

// k_track_drop's sibling for the descriptor views, from the same renumbering table; it runs IN FRONT of k_track_drop (it
// reads the slots and counts that kernel rewrites).  One 64-lane wavefront per track, lane = dimension; a kept view moves
// down past the dropped ones in front of it, and a lane only ever touches its own dimension.
__global__ __launch_bounds__(64) void k_desc_drop(DescStore s, TrackDropArgs p) {
    const size_t row = (size_t)p.rows[blockIdx.x];
    const int M = p.s.count[row];
    float* v = s.views + row * s.V * DESC_DIM + threadIdx.x;
    int w = 0;
    for (int k = 0; k < M; ++k) {
        if (p.remap[p.s.slot[row * p.s.V + k]] < 0) continue;
        if (w != k) v[(size_t)w * DESC_DIM] = v[(size_t)k * DESC_DIM];
        ++w;
    }
}

}  // namespace msckf
