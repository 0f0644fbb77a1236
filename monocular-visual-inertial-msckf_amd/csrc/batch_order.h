// The host's intake of a batch of tracks: what msckf_set_features decides from the CSR integers alone, before
// and beside the device work.  Host code without a HIP header: tests/test_batch_order.py compiles it with the host compiler
// and drives it against a plain-Python model (tests/batch_order_model.py).
//
//   per track     its extent (first slot, last slot, views in slot order), whether it can be split, its view groups.  These
//                 are the rules msckf_exchange_split_rule takes over the WHOLE batch of a sharded update: they exist once, here
//   scan_range    validates the tracks [f0, f1) and writes their sort keys; the first failure of a range is its code, the
//                 lowest failing range decides for the batch.  It never touches a BatchOrder
//   BatchOrder    the pipeline's order of a validated batch: the stable counting sort by (class, first slot, last slot), the
//                 blocks of the split tracks behind the F tracks, the offsets of the K4 blocks, k_gather's and k_feature's
//                 records.  build() clears `valid` first and sets it last: after a failure the value describes no batch
//   layouts       the bytes of the raw image (input order, pinned and in HBM) and of the sorted image k_gather writes
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace msckf {

constexpr int SPLIT_MAXG = 6;            // groups per long track
constexpr int SPLIT_GSLOTS = 10;         // clone slots a group may span
constexpr int WIDE_SPAN = SPLIT_GSLOTS;  // a track over more slots is long: split where the batch's plan allows it
constexpr int TILE_SPAN = 15;            // ... and up to this many it still fits the 90-column band tiles unsplit
constexpr int SPLIT_MAXM = 31;           // the most views k_feature<64> holds
constexpr int MID_DIRECT_ROWS = 2048;    // remainder rows of 11 - 15-slot tracks K6-K7 takes as they are (windows k_fold keeps in LDS)

// one entry of the sorted arrays, read by k_gather where the host's sort left it
struct __attribute__((aligned(8))) GatherRec {
    int f;                        // input index of the track at this sorted position
    int a;                        // its first view in the caller's arrays
    int M;                        // views
    int o;                        // its first view in the sorted arrays
    long long blk;                // offset of its K4 block
};
static_assert(sizeof(GatherRec) == 24 && alignof(GatherRec) == 8, "k_gather reads a record as three 8-byte words");
static_assert(offsetof(GatherRec, f) == 0 && offsetof(GatherRec, a) == 4 && offsetof(GatherRec, M) == 8 &&
              offsetof(GatherRec, o) == 12 && offsetof(GatherRec, blk) == 16, "GatherRec layout");

// one split long track (k_feature.h: two-level nullspace basis)
struct __attribute__((aligned(8))) SplitRec {
    int child[SPLIT_MAXG];               // block index (K5 order) of group g's narrow block; -1: a one-view group has none
    int wide;                            // block index of the remainder block
    unsigned char gv[SPLIT_MAXG + 1];    // group g = views [gv[g], gv[g + 1]) of the track (views in slot order)
    unsigned char ng;                    // groups (>= 2)
    int rows_cap;                        // 3 ng: the rows the remainder block may hold (its place in the dense matrix is found by k_rem_scatter)
};
static_assert(sizeof(SplitRec) == 40 && alignof(SplitRec) == 8, "SplitRec layout");
static_assert(offsetof(SplitRec, child) == 0 && offsetof(SplitRec, wide) == 24 && offsetof(SplitRec, gv) == 28 &&
              offsetof(SplitRec, ng) == 35 && offsetof(SplitRec, rows_cap) == 36, "SplitRec layout");

// ---- per track -------------------------------------------------------------------------------------------------------------
struct TrackExtent {
    int lo, hi;                   // first and last clone slot
    bool ordered = true;          // views in ascending slot order (the groups of a split are view ranges)
    explicit TrackExtent(int N) : lo(N), hi(-1) {}
    void add(int sl) {
        if (sl < hi) ordered = false;
        lo = std::min(lo, sl); hi = std::max(hi, sl);
    }
    int span() const { return hi - lo + 1; }
};

inline TrackExtent track_extent(const int32_t* slots, int M, int N) {
    TrackExtent e(N);
    for (int i = 0; i < M; ++i) e.add(slots[i]);
    return e;
}

// stretches of at most SPLIT_GSLOTS slots a span is cut into
inline int split_stretches(int span) { return (span + SPLIT_GSLOTS - 1) / SPLIT_GSLOTS; }

// a long track that can be split: views in slot order, no more than k_feature<64> holds, no more groups than a SplitRec names
inline bool splittable(const TrackExtent& e, int M) {
    return e.span() > WIDE_SPAN && e.ordered && M <= SPLIT_MAXM && split_stretches(e.span()) <= SPLIT_MAXG;
}

// The view groups of a split track: fn(g, v0, v1) for group g, the views [v0, v1), of every stretch that has one, in order.
// Returns their number.  (Stretch g0 is the slots below lo + (g0 + 1) span / ng0: at most ceil(span / ng0) <= 10 of them.)
template <class Fn>
inline int for_each_group(int lo, int span, const int32_t* slots, int M, Fn&& fn) {
    const int ng0 = split_stretches(span);
    int ng = 0, v = 0;
    for (int g0 = 0; g0 < ng0; ++g0) {
        const int bnd = lo + (int)(((long long)(g0 + 1) * span) / ng0);
        const int v0 = v;
        while (v < M && slots[v] < bnd) ++v;
        if (v == v0) continue;                                 // no view in this stretch of slots
        fn(ng, v0, v);
        ++ng;
    }
    return ng;
}

// A batch MOST of whose tracks span 11 - 15 slots and none more (BASELINE configs[4]: every track 15 views) keeps the
// 90-column band pipeline for all of them: split, each would leave 3 remainder rows to the dense tree
// ... and so does one whose remainder rows (6 per such track) would be too many for K6-K7 to take as they are: the 90-column
// pipeline (539 us at 2000 tracks ~ U[2, 15]) beats band pipeline + remainder tree (866 us) there.
// direct_cap: the remainder rows K6-K7 takes as they are at this window; wide_window: wider than k_fold keeps in LDS
inline bool keeps_wide_tiles(int n_mid, int n_long, int F, int direct_cap, bool wide_window) {
    return n_long == 0 && (2 * n_mid > F || 6 * n_mid > (wide_window ? direct_cap : std::min(direct_cap, MID_DIRECT_ROWS)));
}

// ---- the scan ----------------------------------------------------------------------------------------------------------------
constexpr int kOrderOk = 0, kOrderErrArg = -1, kOrderErrDupSlot = -6;   // MSCKF_OK, MSCKF_ERR_ARG, MSCKF_ERR_DUP_SLOT

struct ScanPart {
    int err = kOrderOk;
    int Mmax[3] = {0, 0, 0};      // most views of a track, per class
    int n_mid = 0, n_long = 0;    // tracks of 11 - 15 slots / of more (any class)
    void add(const ScanPart& o) {
        for (int k = 0; k < 3; ++k) Mmax[k] = std::max(Mmax[k], o.Mmax[k]);
        n_mid += o.n_mid; n_long += o.n_long;
    }
    int Mmax_all() const { return std::max(Mmax[0], std::max(Mmax[1], Mmax[2])); }
};

// Validates the tracks [f0, f1) and writes key_in[f], M_in[f] for them.  key = (class, first slot, last slot); class 0: tracks
// of up to WIDE_SPAN clone slots and long ones that cannot be split; class 2: long tracks, split (`split`: the context's
// verdict).  After a failure the range's outputs are not to be read.
inline ScanPart scan_range(int N, int maxM, bool split, const int32_t* view_ptr, const int32_t* obs_slot, int f0, int f1,
                           int* key_in, unsigned char* M_in) {
    ScanPart out, fail;
    const size_t NN = (size_t)N * N;
    for (int f = f0; f < f1; ++f) {
        const int a = view_ptr[f], b = view_ptr[f + 1], M = b - a;
        if (M < 1 || M > maxM) { fail.err = kOrderErrArg; return fail; }
        TrackExtent e(N);
        unsigned long long seen = 0;    // N <= 64 fast path; general check below
        for (int i = a; i < b; ++i) {
            const int sl = obs_slot[i];
            if (sl < 0 || sl >= N) { fail.err = kOrderErrArg; return fail; }
            e.add(sl);
            if (N <= 64) {
                if (seen & (1ull << sl)) { fail.err = kOrderErrDupSlot; return fail; }
                seen |= 1ull << sl;
            } else {
                for (int k = a; k < i; ++k) if (obs_slot[k] == sl) { fail.err = kOrderErrDupSlot; return fail; }
            }
        }
        const int span = e.span();
        if (span > TILE_SPAN) ++out.n_long; else if (span > WIDE_SPAN) ++out.n_mid;
        const int cls = (split && splittable(e, M)) ? 2 : 0;
        key_in[f] = (int)(cls * NN + (size_t)e.lo * N + e.hi);
        M_in[f] = (unsigned char)M;
        out.Mmax[cls] = std::max(out.Mmax[cls], M);
    }
    return out;
}

// keeps_wide_tiles() said so: no track of the batch is split after all
inline void drop_split_class(int N, int F, int* key_in, ScanPart& tot) {
    const size_t NN = (size_t)N * N;
    for (int f = 0; f < F; ++f) key_in[f] = (int)((size_t)key_in[f] % NN);
    tot.Mmax[0] = tot.Mmax_all(); tot.Mmax[2] = 0;
}

// ---- the layouts -------------------------------------------------------------------------------------------------------------
// raw image (input order): doubles first, then the ints; behind the arrays the sort's records: one GatherRec per entry of the
// sorted arrays -- the tracks and, for long tracks that are split, their blocks: a narrow block per view group of 2+ views and
// one remainder block, i.e. at most M / 2 + 1 per track (a ragged track may span 11+ slots with three views) -- and one
// SplitRec per long track
struct RawLayout {
    size_t r_uv, r_base, r_m, r_rho, r_slot;
    size_t raw_bytes;             // the arrays (a multiple of 16, as r_base is)
    size_t rec_cap;               // GatherRecs there is room for
    size_t pin_bytes;
    size_t split_off(int Fs) const { return raw_bytes + (((size_t)Fs * sizeof(GatherRec) + 15) & ~(size_t)15); }   // the SplitRecs
};

inline RawLayout raw_layout(int F, int sumM) {
    RawLayout l;
    l.r_uv = 0; l.r_base = l.r_uv + (size_t)sumM * 16; l.r_m = l.r_base + (size_t)F * 24; l.r_rho = l.r_m + (size_t)F * 24;
    l.r_slot = l.r_rho + (size_t)F * 8;
    l.raw_bytes = (l.r_slot + (size_t)sumM * 4 + 15) & ~(size_t)15;
    l.rec_cap = 2 * (size_t)F + (size_t)sumM / 2 + 8;
    l.pin_bytes = l.raw_bytes + l.rec_cap * sizeof(GatherRec) + ((size_t)F + 1) * sizeof(SplitRec);
    return l;
}

// sorted image (what the kernels read), written by k_gather: Fs entries, sumMs views
struct SortedLayout {
    size_t o_uv, o_base, o_m, o_rho, o_blk, o_view;
    size_t o_perm;                // sorted position -> input index
    size_t o_slot, o_fmin;
    size_t o_info;                // FeatInfo records (16-byte aligned)
    size_t feat_bytes;
};

inline SortedLayout sorted_layout(int Fs, int sumMs, size_t info_bytes) {
    SortedLayout l;
    l.o_uv = 0; l.o_base = l.o_uv + (size_t)sumMs * 16; l.o_m = l.o_base + (size_t)Fs * 24; l.o_rho = l.o_m + (size_t)Fs * 24;
    l.o_blk = l.o_rho + (size_t)Fs * 8; l.o_view = l.o_blk + (size_t)Fs * 8;
    l.o_perm = l.o_view + (((size_t)(Fs + 1) * 4 + 7) & ~(size_t)7);
    l.o_slot = (l.o_perm + (size_t)Fs * 4 + 7) & ~(size_t)7; l.o_fmin = l.o_slot + (((size_t)sumMs * 4 + 7) & ~(size_t)7);
    l.o_info = (l.o_fmin + (size_t)Fs * 4 + 15) & ~(size_t)15;
    l.feat_bytes = l.o_info + (size_t)Fs * info_bytes;
    return l;
}

// ---- the order ---------------------------------------------------------------------------------------------------------------
// Tracks that are split are sorted behind the others ([0, Fb) short, [Fb, F) long); the sorted arrays hold their blocks behind
// the F tracks -- [F, F + nNarrow) the narrow blocks of their view groups (ordinary <= 10-slot tracks to every K5 kernel,
// sorted by (first slot, last slot) among themselves), [F + nNarrow, Fs) one remainder block per long track (3 (groups - 1)
// rows that touch every slot of the track).  The long tracks themselves, [Fb, F), are entries of K1-K3 only (gate, mask,
// counters): no K5 plan names them.
struct BatchOrder {
    enum Fail { kBuilt = 0, kRecordCapacity, kRemainderCapacity };

    bool valid = false;           // the members below describe the batch build() was last called for
    int Fb = 0, Fw = 0;           // short tracks; long tracks, split
    int Fs = 0, nNarrow = 0;      // entries of the sorted arrays; narrow blocks
    int sumMs = 0;                // views of all entries
    bool split_on = false;        // this batch's long tracks were split (Fw > 0: k_feature<64, true> writes their blocks)
    int rem_cap = 0;              // rows the remainder blocks may hold in all (3 per view group)
    int Mmax = 0, Mmax_band = 0, Mmax_wide = 0;      // most views of a track: of all, of [0, Fb), of [Fb, F)
    long long stack_elems = 0;    // elements of the K4 blocks of all entries
    std::vector<int> perm;        // [F] sorted position -> input index
    std::vector<int> h_view;      // [Fs + 1] CSR offsets of the sorted arrays
    std::vector<int> h_fmin, h_fmax;                 // [Fs] first / last slot of an entry
    std::vector<int> h_parent;    // [Fs - F] sorted index of the long track a block belongs to
    std::vector<SplitRec> h_split;                   // per long track, in sorted order

    // the batch without tracks
    void reset() {
        Fb = Fw = Fs = nNarrow = sumMs = rem_cap = Mmax = Mmax_band = Mmax_wide = 0;
        split_on = false; stack_elems = 0;
        perm.clear(); h_view.assign(1, 0); h_fmin.clear(); h_fmax.clear(); h_parent.clear(); h_split.clear();
        valid = true;
    }

    // key_in, M_in, tot: of scan_range over [0, F) (after drop_split_class where it applies).  rec: room for rec_cap records;
    // rem_rows_cap: the remainder rows a record of the group exchange takes (msckf_set_exchange_split), < 0 where none does.
    Fail build(int N, int F, const int32_t* view_ptr, const int32_t* obs_slot, const int* key_in, const unsigned char* M_in,
               const ScanPart& tot, size_t rec_cap, int rem_rows_cap, GatherRec* rec) {
        valid = false;
        const size_t NN = (size_t)N * N;
        Mmax = tot.Mmax_all();
        // counting sort by the key: stable, O(F + N^2); the short tracks first, the long ones behind them
        perm.resize(F);
        h_fmin.resize(F); h_fmax.resize(F);
        cnt_.assign(3 * NN + 1, 0);
        for (int f = 0; f < F; ++f) cnt_[key_in[f] + 1]++;
        // first / last slot of the sorted tracks: a run per occupied key
        for (size_t k = 0, pos = 0; k < 3 * NN; ++k) {
            const int n = cnt_[k + 1];
            if (n == 0) continue;
            const int lo = (int)((k % NN) / N), hi = (int)(k % N);
            std::fill(h_fmin.begin() + pos, h_fmin.begin() + pos + n, lo);
            std::fill(h_fmax.begin() + pos, h_fmax.begin() + pos + n, hi);
            pos += n;
        }
        for (size_t i = 1; i < cnt_.size(); ++i) cnt_[i] += cnt_[i - 1];
        Fb = cnt_[NN];                                                   // short tracks: sorted positions [0, Fb)
        Fw = F - Fb;                                                     // long tracks, split: [Fb, F)
        for (int f = 0; f < F; ++f) perm[cnt_[key_in[f]]++] = f;
        Mmax_band = tot.Mmax[0]; Mmax_wide = tot.Mmax[2];
        split_on = Fw > 0;
        // ---- the blocks of the long tracks (k_feature.h): view groups of at most SPLIT_GSLOTS slots -> narrow blocks, one
        //      remainder block per track
        h_split.clear(); h_parent.clear();
        narrow_.clear(); wide_.clear();
        rem_cap = 0;
        if (split_on) {
            h_split.resize(Fw);
            for (int sidx = Fb; sidx < F; ++sidx) {
                const int f = perm[sidx], a = view_ptr[f], M = M_in[f], lo = h_fmin[sidx], hi = h_fmax[sidx], pi = sidx - Fb;
                SplitRec sr{};
                for (int g = 0; g < SPLIT_MAXG; ++g) sr.child[g] = -1;
                const int ng = for_each_group(lo, hi - lo + 1, obs_slot + a, M, [&](int g, int v0, int v1) {
                    sr.gv[g] = (unsigned char)v0;
                    if (v1 - v0 >= 2) narrow_.push_back({sidx, f, a + v0, v1 - v0, obs_slot[a + v0], obs_slot[a + v1 - 1], pi, g});
                });
                sr.gv[ng] = (unsigned char)M; sr.ng = (unsigned char)ng;
                sr.rows_cap = 3 * ng; rem_cap += 3 * ng;
                h_split[pi] = sr;
                wide_.push_back({sidx, f, a, M, lo, hi, pi, -1});
            }
            // the narrow blocks among themselves by (first slot, last slot): the band plan walks them as a second run
            cnt_.assign(NN + 1, 0);
            for (const Blk& b : narrow_) cnt_[(size_t)b.lo * N + b.hi + 1]++;
            for (size_t i = 1; i < cnt_.size(); ++i) cnt_[i] += cnt_[i - 1];
            sorted_.resize(narrow_.size());
            for (const Blk& b : narrow_) sorted_[cnt_[(size_t)b.lo * N + b.hi]++] = b;
            narrow_.swap(sorted_);
        }
        nNarrow = (int)narrow_.size();
        if ((size_t)F + narrow_.size() + wide_.size() > rec_cap) return kRecordCapacity;
        // split records: the rows go to the record's remainder section, whose capacity every rank was told
        if (split_on && rem_rows_cap >= 0 && rem_cap > rem_rows_cap) return kRemainderCapacity;
        Fs = F + (int)narrow_.size() + (int)wide_.size();
        h_view.resize(Fs + 1); h_fmin.resize(Fs); h_fmax.resize(Fs);
        h_parent.resize(Fs - F);
        // the sorted CSR offsets and the offsets of the K4 blocks: a prefix over the sorted order; k_gather's records
        long long blk = 0;
        int pos = 0;
        for (int sidx = 0; sidx < F; ++sidx) {
            const int f = perm[sidx], M = M_in[f];
            h_view[sidx] = pos;
            const bool parent = split_on && sidx >= Fb;                  // (a split track has no block of its own)
            rec[sidx] = GatherRec{f, view_ptr[f], M, pos, parent ? 0 : blk};
            if (!parent) blk += (long long)(6 * M + 1) * (2 * M);
            pos += M;
        }
        int e = F;
        for (const Blk& b : narrow_) {
            h_view[e] = pos; h_fmin[e] = b.lo; h_fmax[e] = b.hi; h_parent[e - F] = b.parent;
            rec[e] = GatherRec{b.f, b.a, b.M, pos, blk};
            h_split[b.pi].child[b.g] = e;
            blk += (long long)(6 * b.M + 1) * (2 * b.M);
            pos += b.M; ++e;
        }
        for (const Blk& b : wide_) {
            h_view[e] = pos; h_fmin[e] = b.lo; h_fmax[e] = b.hi; h_parent[e - F] = b.parent;
            rec[e] = GatherRec{b.f, b.a, b.M, pos, blk};
            h_split[b.pi].wide = e;
            blk += (long long)(6 * b.M + 1) * (3 * SPLIT_MAXG);
            pos += b.M; ++e;
        }
        h_view[Fs] = pos;
        sumMs = pos;
        stack_elems = blk;
        valid = true;
        return kBuilt;
    }

private:
    struct Blk { int parent, f, a, M, lo, hi, pi, g; };
    std::vector<int> cnt_;                           // (scratch; like the members above it keeps its capacity between calls)
    std::vector<Blk> narrow_, wide_, sorted_;
};

}  // namespace msckf
