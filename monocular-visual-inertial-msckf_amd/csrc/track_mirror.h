// The host's integer mirror of the resident track store: which id sits in which row, the clone slots of every
// row's views, the anchor, the lost_for / tracked_for counters, the creation number, the free rows and "every view has a
// descriptor".  Every msckf_tracks_* call decides from it what the device does.  Host code without a HIP header:
// tests/test_track_mirror.py compiles it with the host compiler and drives it against a plain-Python model.
//
// The contract:
//   rows      row 0 goes out first; freed rows are reused last-in first-out
//   intake    plan() is const: it names the first offending pair and its code, or one (row, position, fresh) per pair; commit()
//             applies one pair.  A call that fails in plan() leaves every member as it was
//   counters  zero on creation and when a row is freed; commit() and age_unlisted() are the only other writers
//   creation  numbers come from a counter that only clear() resets (rows are recycled: the reference's dict order)
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

struct TrackPlace { int row, pos, fresh; };   // where a pair's view goes: position pos of row; fresh: the row is handed out for it

class TrackMirror {
public:
    static constexpr int kOk = 0, kErrArg = -1, kErrDupSlot = -6;   // MSCKF_OK, MSCKF_ERR_ARG, MSCKF_ERR_DUP_SLOT

    // ---- sizing and clearing -----------------------------------------------------------------------------------------
    void size(int T, int V) {
        T_ = T; V_ = V;
        id_.assign(T, -1); M_.assign(T, 0); anchor_.assign(T, -1); slots_.assign((size_t)T * V, 0);
        lost_.assign(T, 0); tracked_.assign(T, 0); seq_.assign(T, 0); hasdesc_.assign(T, 0); mark_.assign(T, 0);
        clear();
    }
    void clear() {                        // (harmless before size(): no rows)
        row_of_.clear(); dropped_.clear();
        views_ = 0; next_seq_ = 0;
        std::fill(id_.begin(), id_.end(), -1);
        std::fill(M_.begin(), M_.end(), 0);
        std::fill(lost_.begin(), lost_.end(), 0);
        std::fill(tracked_.begin(), tracked_.end(), 0);
        std::fill(hasdesc_.begin(), hasdesc_.end(), 0);
        free_.resize(T_);
        for (int r = 0; r < T_; ++r) free_[r] = T_ - 1 - r;          // row 0 goes out first
    }

    // ---- lookup ------------------------------------------------------------------------------------------------------
    int rows() const { return T_; }
    int row_of(int id) const { const auto it = row_of_.find(id); return it == row_of_.end() ? -1 : it->second; }
    int id(int r) const { return id_[r]; }                           // -1: the row is free
    int M(int r) const { return M_[r]; }
    const int* slots(int r) const { return &slots_[(size_t)r * V_]; }   // M(r) clone slots, ascending
    int anchor(int r) const { return anchor_[r]; }                   // -1: frozen
    int lost(int r) const { return lost_[r]; }                       // lost_for_n_frames (MSCKF.py:400, :438)
    int tracked(int r) const { return tracked_[r]; }                 // tracked_for_n_frames (:411-412)
    long long seq(int r) const { return seq_[r]; }
    bool hasdesc(int r) const { return hasdesc_[r] != 0; }           // every view of the row came with a descriptor
    int n_tracks() const { return (int)row_of_.size(); }
    long long n_views() const { return views_; }
    const std::vector<int>& dropped() const { return dropped_; }     // ids the last drop_clones() deleted
    const std::vector<int>& free_rows() const { return free_; }      // a stack: back() goes out next
    bool all_have_desc() const {
        for (int r = 0; r < T_; ++r) if (id_[r] >= 0 && !hasdesc_[r]) return false;
        return true;
    }

    // ---- intake ------------------------------------------------------------------------------------------------------
    // The views (ids[i], newest clone), i < n.  Each pair is checked in this order and the first offending pair in list order
    // decides: a negative id or !pair_ok(i) kErrArg; an id listed twice or a view already in the newest clone kErrDupSlot; a
    // full row kErrArg.  After the loop: more fresh ids than free rows, kErrArg (*bad: the first fresh pair without a row).
    // kOk: out[i] for every pair; fresh pairs take the rows the free stack hands out next, in listed order.
    template <class PairOk>
    int plan(const int32_t* ids, int n, int newest, TrackPlace* out, int* bad, PairOk pair_ok) const {
        std::unordered_set<int> seen;
        size_t taken = 0;
        int over = -1;
        auto fail = [&](int i, int code) { if (bad) *bad = i; return code; };
        for (int i = 0; i < n; ++i) {
            if (ids[i] < 0 || !pair_ok(i)) return fail(i, kErrArg);
            if (!seen.insert(ids[i]).second) return fail(i, kErrDupSlot);
            const int r = row_of(ids[i]);
            if (r < 0) {
                if (taken < free_.size()) out[i] = TrackPlace{free_[free_.size() - 1 - taken], 0, 1};
                else if (over < 0) over = i;
                ++taken;
                continue;
            }
            const int M = M_[r];
            if (M > 0 && slots_[(size_t)r * V_ + M - 1] == newest) return fail(i, kErrDupSlot);
            if (M + 1 > V_) return fail(i, kErrArg);
            out[i] = TrackPlace{r, M, 0};
        }
        if (over >= 0) return fail(over, kErrArg);
        return kOk;
    }
    int plan(const int32_t* ids, int n, int newest, TrackPlace* out, int* bad = nullptr) const {
        return plan(ids, n, newest, out, bad, [](int) { return true; });
    }

    // One planned pair, in listed order.  A fresh pair creates the track first: anchor = newest, counters 0, the next creation
    // number.  view: the view goes in (tracked + 1, lost = 0); else the match failed (lost + 1, no view: a track created so
    // stays live without one).  with_desc: the caller stores a descriptor with the view.
    void commit(int id, const TrackPlace& p, int newest, bool view, bool with_desc) {
        const int r = p.row;
        if (p.fresh) {
            free_.pop_back();             // (r: plan() handed the rows out in this order)
            row_of_.emplace(id, r);
            id_[r] = id; M_[r] = 0; anchor_[r] = newest;
            seq_[r] = next_seq_++;
            tracked_[r] = 0; lost_[r] = 0;
            hasdesc_[r] = with_desc;
        }
        if (!view) { ++lost_[r]; return; }                           // MSCKF.py:400
        if (!with_desc) hasdesc_[r] = 0;
        slots_[(size_t)r * V_ + M_[r]++] = newest;                   // appended (:403-421) or created (:424-436)
        ++views_;
        ++tracked_[r]; lost_[r] = 0;                                 // :411-412
    }

    // lost + 1 for every live row the frame did not list (MSCKF.py:438)
    void age_unlisted(const TrackPlace* listed, int n) {
        std::fill(mark_.begin(), mark_.end(), 0);
        for (int i = 0; i < n; ++i) mark_[listed[i].row] = 1;
        for (int r = 0; r < T_; ++r) if (id_[r] >= 0 && !mark_[r]) ++lost_[r];
    }

    // ---- freeing -----------------------------------------------------------------------------------------------------
    // all or nothing: an id that is not live, or listed twice, and nothing is removed
    int remove(const int32_t* ids, int n) {
        std::unordered_set<int> seen;
        for (int i = 0; i < n; ++i)
            if (!row_of_.count(ids[i]) || !seen.insert(ids[i]).second) return kErrArg;
        for (int i = 0; i < n; ++i) free_row(row_of(ids[i]));
        return kOk;
    }

    // msckf_remove_clones (MSCKF.py:760-779): remap[s] = the new slot of clone s, -1 if it goes (monotone).  Slots and anchors
    // are renumbered; a row left without a view is freed and its id recorded in dropped(), in ascending row order.
    void forget_dropped() { dropped_.clear(); }                      // (a removal of clones from an empty store)
    void drop_clones(const short* remap) {
        dropped_.clear();
        for (int r = 0; r < T_; ++r) {
            if (id_[r] < 0) continue;
            int* sl = &slots_[(size_t)r * V_];
            int M = 0;
            for (int v = 0; v < M_[r]; ++v) if (remap[sl[v]] >= 0) sl[M++] = remap[sl[v]];
            views_ -= M_[r] - M;
            M_[r] = M;
            if (anchor_[r] >= 0) anchor_[r] = remap[anchor_[r]];
            if (M == 0) { dropped_.push_back(id_[r]); free_row(r); }
        }
    }

    // ---- enumeration -------------------------------------------------------------------------------------------------
    void live_rows(std::vector<int>& out) const {                    // in row order
        out.clear();
        for (int r = 0; r < T_; ++r) if (id_[r] >= 0) out.push_back(r);
    }
    void live_rows_by_creation(std::vector<int>& out) const {        // the reference's dict order
        by_creation(out, [](int) { return true; });
    }
    // ... those with a view in a clone slot s with want[s] != 0
    void live_rows_by_creation(const std::vector<char>& want, std::vector<int>& out) const {
        by_creation(out, [&](int r) {
            const int* sl = slots(r);
            for (int v = 0; v < M_[r]; ++v) if (want[sl[v]]) return true;
            return false;
        });
    }

    // ---- consistency -------------------------------------------------------------------------------------------------
    // the device's count / anchor / slot[] of row r, in a window of N clones, against the mirror
    bool agrees(int r, int count, int anchor, const int* slot, int N) const {
        bool same = count == M_[r] && anchor == anchor_[r] && anchor < N;
        for (int v = 0; same && v < M_[r]; ++v) same = slot[v] == slots_[(size_t)r * V_ + v] && slot[v] >= 0 && slot[v] < N;
        return same;
    }

private:
    void free_row(int r) {
        row_of_.erase(id_[r]);
        views_ -= M_[r];
        id_[r] = -1; M_[r] = 0;
        lost_[r] = tracked_[r] = 0;       // the counters die with the track
        hasdesc_[r] = 0;
        free_.push_back(r);
    }
    template <class Pred>
    void by_creation(std::vector<int>& out, Pred keep) const {
        std::vector<std::pair<long long, int>> live;                 // (creation number, row)
        for (int r = 0; r < T_; ++r) if (id_[r] >= 0 && keep(r)) live.emplace_back(seq_[r], r);
        std::sort(live.begin(), live.end());
        out.clear();
        for (const auto& e : live) out.push_back(e.second);
    }

    int T_ = 0, V_ = 0;
    std::vector<int> id_, M_, anchor_, slots_;                       // per row: id (-1: free), views, anchor slot, [row][V] slots
    std::vector<int> lost_, tracked_;
    std::vector<long long> seq_;                                     // per row: when the track was created
    long long next_seq_ = 0;
    std::vector<int> free_, dropped_;
    std::unordered_map<int, int> row_of_;                            // id -> row
    long long views_ = 0;
    std::vector<char> hasdesc_, mark_;                               // (mark_: age_unlisted's scratch)
};
