// The sweep kernels' schedules and tables (k_sweep.h, k_wsweep.h), made by the host: each fold's first macro step, the rows of
// R that are final at the head of every step, which producer rows a step waits for, what a ring sweep publishes -- and the
// root node of a plan with the tables of the merge level that rides in its launch.  Functions of the folds' shapes alone.
// The fused launches wait inside the launch on what these tables say: a wrong entry is a workgroup that waits for a row
// which never comes.  Standard headers only: tests/sweep_plan_driver.cpp builds this file with the host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace msckf {

struct SweepFold {
    long long src_off;   // offset (doubles) of the source block in rbuf: row-major w x (w+1), upper triangular
    int off;             // first column of the source window, local to the node
    int w;               // rows / columns of the source triangle (<= SWEEP_MAX_W)
    int ew;              // tile width: columns [off, off+ew) may fill in (w <= ew <= SWEEP_MAX_W)
    int t0;              // macro step of the fold's first column
    int prod;            // 0, or 1 + index of the progress word of the node that is still WRITING the source block in the same
                         // launch (k_root_gain's merge workgroups): the flusher lets a macro step start only when the rows its
                         // folds fetch in it are published (host table, sweep_gate_table)
    int ld;              // doubles per row of the source block (0: w + 1).  A streamed block has whole cache lines per row (64):
                         // a line fetched for a published row must not hold part of a row that is not final yet
};

struct SweepNode {
    int fold_begin, fold_end;   // folds [begin, end); a first fold with t0 == 0 is adopted (copied into R), the others
                                // run on fold slot (i - first scheduled) % NF
    int wtot;                   // columns of the node's R
    int nsteps;                 // macro steps
    long long out_off;          // output block in rbuf: row-major wtot x (wtot+1), or wtot x ldo
    int ldo;                    // doubles per row of the output block (0: wtot + 1)
    int prod_base;              // streamed sources: SweepFold::prod counts from progress word src_progress[prod_base]
    int n_gate;                 // ... the step-0 requirements behind this node's own gate table (SweepArgs::gate_per_node)
    int pad;
};

constexpr int SWEEP_MAX_W = 60;        // widest source / envelope (local column 63 holds the rhs)
constexpr int WS_PUB_LAG = 4;          // k_wsweep: steps between a row's store and the wait for it (the count goes out one step later)
constexpr int SWEEP_PLAN_NF = 8;       // fold slots of a sweep workgroup unless the caller says otherwise (SWEEP_NW)

inline void sweep_schedule(std::vector<SweepFold>& folds, int begin, int end, int* nsteps, int nf = SWEEP_PLAN_NF, bool adopt = true) {
    int last = 0;
    if (end > begin && adopt) folds[begin].t0 = 0;         // adopted: copied into the empty R, no elimination steps
    const int first = adopt ? begin + 1 : begin;           // (not adopted: a streamed first triangle is folded like the others)
    for (int g = first; g < end; ++g) {
        int t0 = 1;                                        // step t0 - 1 publishes the fold's first column
        if (g > first) t0 = folds[g - 1].t0 + (folds[g].off - folds[g - 1].off) + 1;
        // (a fold runs one step per column of its ENVELOPE ew >= w: where R already reaches further right than the
        //  source triangle, the tile's rows fill in there and the fill has to be eliminated as well)
        if (g - first >= nf) t0 = std::max(t0, folds[g - nf].t0 + folds[g - nf].ew + 1);
        folds[g].t0 = t0;
        last = std::max(last, t0 + folds[g].ew);
    }
    *nsteps = last;
}

// Rows of R no present or future fold step touches at the head of macro step t (the schedule is static).  Entry
// t = lo | n << 16: rows [lo, lo + n) are final (k_wsweep: leave the ring) at the head of step t; entry nsteps covers the
// rest.  Returns false when some step would touch a row whose slot in a ring of rc rows still holds an unflushed row.
inline bool sweep_flush_table(const std::vector<SweepFold>& folds, int begin, int end, int nsteps, int wtot, int rc,
                              std::vector<int>& tab) {
    const int first = (end > begin && folds[begin].t0 == 0) ? begin + 1 : begin;   // an adopted triangle runs no step
    int lprev = 0;
    bool ok = true;
    for (int t = 0; t <= nsteps; ++t) {
        int L = wtot, H = -1;
        if (t < nsteps) {
            for (int g = first; g < end; ++g) {
                const SweepFold& f = folds[g];
                if (t >= f.t0 + f.ew) continue;                           // finished (one step per envelope column)
                const int row = f.off + std::max(0, t - f.t0);            // its present (or first) pivot row
                L = std::min(L, row);
                if (t >= f.t0) H = std::max(H, row);
            }
        }
        L = std::max(L, lprev);
        if (H >= lprev + rc) ok = false;                                  // a touched row aliases one flushed in this step
        if (t == 0 && first > begin && folds[begin].off + folds[begin].w > rc) ok = false;   // the adopted rows fit the ring
        tab.push_back(lprev | ((L - lprev) << 16));
        lprev = L;
    }
    return ok;
}

// Streamed sources of a node (SweepFold::prod, k_root_gain's merge workgroups): which rows of which producer the fold
// wavefronts fetch at the head of which macro step -- k_sweep.h fetches rows [0, 8) of a fold's source before step 0 (the first
// nf folds) or in chunk max((ew' - 1) / 8 - 1, 0) of the fold that has the slot before it, and rows [8 KK + 8, 8 KK + 16) at
// the head of the fold's chunk KK.  Appended to `tab`: nsteps + 2 step entries (up to two requirements prod << 6 | rows, 12 bits
// each; a third moves to an earlier step, which only asks for it sooner) | the requirements of step 0.  Returns their count.
inline int sweep_gate_table(const std::vector<SweepFold>& folds, int begin, int end, int nsteps, int nf, std::vector<int>& tab) {
    const int first = (end > begin && folds[begin].t0 == 0) ? begin + 1 : begin;
    // (step, requirement) pairs, then a sort by step: no per-step containers on the one-shot call's host path
    static thread_local std::vector<std::pair<int, int>> req;
    req.clear();
    for (int i = first; i < end; ++i) {
        const SweepFold& f = folds[i];
        if (f.prod <= 0) continue;
        int step = 0;
        if (i - first >= nf) { const SweepFold& q = folds[i - nf]; step = q.t0 + 8 * std::max((q.ew - 1) / 8 - 1, 0); }
        req.push_back({std::min(step, nsteps), ((f.prod - 1) << 6) | std::min(f.w, 8)});
        for (int kk = 0; kk < 8 && 8 * kk < f.ew; ++kk)
            if (8 * kk + 8 < f.w) req.push_back({std::min(f.t0 + 8 * kk, nsteps), ((f.prod - 1) << 6) | std::min(f.w, 8 * kk + 16)});
    }
    std::sort(req.begin(), req.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.first > y.first; });   // latest step first
    const size_t base = tab.size();
    tab.resize(base + nsteps + 2, 0);
    std::vector<int> step0;
    int carry[64], ncarry = 0;                      // requirements pushed to an earlier step (a step takes two)
    size_t k = 0;
    for (int t = nsteps + 1; t >= 0; --t) {
        int mine[2], n = 0;
        auto take = [&](int r) { if (t == 0) step0.push_back(r); else if (n < 2) mine[n++] = r; else if (ncarry < 64) carry[ncarry++] = r; else step0.push_back(r); };
        const int nc = ncarry; ncarry = 0;
        int prev[64];
        for (int j = 0; j < nc; ++j) prev[j] = carry[j];
        for (int j = 0; j < nc; ++j) take(prev[j]);
        while (k < req.size() && req[k].first == t) take(req[k++].second);
        if (t > 0) tab[base + t] = (n > 0 ? mine[0] : 0) | (n > 1 ? mine[1] << 12 : 0);
    }
    tab.insert(tab.end(), step0.begin(), step0.end());
    return (int)step0.size();
}

// k_wsweep with PUB: what wavefront 0 publishes at the head of macro step t -- the rows that were final WS_PUB_LAG + 1 steps
// earlier, where that count passes a boundary of k_gstream.h's 16-row blocks (they end at rows = wtot mod 16); 0: nothing.
// Appended behind the node's flush entries (tab[off .. off + nsteps]).
inline void sweep_publish_table(std::vector<int>& tab, size_t off, int nsteps, int wtot) {
    const int boff = (16 - (wtot & 15)) & 15;
    int published = 0;
    for (int t = 0; t <= nsteps; ++t) {
        int pr = 0;
        if (t > WS_PUB_LAG) {
            const int e = tab[off + t - WS_PUB_LAG - 1];
            const int rows = (e & 0xFFFF) + (e >> 16);
            if (((rows + boff) >> 4) > ((published + boff) >> 4)) { pr = rows; published = rows; }
        }
        tab.push_back(pr);
    }
}

// The ring form's tables (k_wsweep): per node the flush table, then the publish table, appended to `tab`; `offs` gets where each
// node's begin.  False: a node's band does not fit a ring of rc rows.
inline bool sweep_ring_tables(const std::vector<SweepFold>& folds, const SweepNode* nodes, size_t n, int rc, std::vector<int>& tab,
                              std::vector<int>& offs) {
    for (size_t i = 0; i < n; ++i) {
        const SweepNode& nd = nodes[i];
        const size_t o = tab.size();
        offs.push_back((int)o);
        if (!sweep_flush_table(folds, nd.fold_begin, nd.fold_end, nd.nsteps, nd.wtot, rc, tab)) return false;
        sweep_publish_table(tab, o, nd.nsteps, nd.wtot);
    }
    return true;
}

// A sweep node's schedule and tables depend on its folds' shapes, not on where its sources lie or how many tracks they hold:
// a window's group shape repeats from batch to batch, and most merge nodes of one plan share a shape.  Kept by the exact inputs
// (key: wtot, fold slots, adopted, gate table wanted, then off, w, ew, prod, ld of every fold), so a hit IS the table a rebuild gives.
struct SweepTables {
    std::vector<int> key;
    std::vector<int> t0;                  // SweepFold::t0 of the folds (sweep_schedule)
    int nsteps = 0;
    std::vector<int> tab;                 // sweep_flush_table, then sweep_gate_table where the key asks for it
    int n_gate = -1;                      // ... its step-0 requirements; -1: no gate table
};
struct SweepMemo {
    static constexpr int CAP = 64;
    std::vector<SweepTables> e;           // up to CAP, the oldest replaced first
    int next = 0;
    std::vector<int> key;                 // (scratch)
};

// Schedule and tables of the node with folds [begin, end): t0 of the folds and *nsteps are set, the returned entry of the memo
// holds the flush table (every row final at the head of which macro step) and, with `gate`, the gate table behind it.  From the
// memo where the same folds were seen before (*hit); else the entry is written anew, over the oldest one when the memo is full.
inline int sweep_tables(SweepMemo& m, std::vector<SweepFold>& folds, int begin, int end, int wtot, int nf, bool adopt, bool gate,
                        int* nsteps, bool* hit = nullptr) {
    std::vector<int>& key = m.key;
    key.clear();
    key.push_back(wtot); key.push_back(nf); key.push_back(adopt ? 1 : 0); key.push_back(gate ? 1 : 0);
    for (int g = begin; g < end; ++g) {
        const SweepFold& f = folds[g];
        key.push_back(f.off); key.push_back(f.w); key.push_back(f.ew); key.push_back(f.prod); key.push_back(f.ld);
    }
    for (size_t i = 0; i < m.e.size(); ++i) {
        const SweepTables& t = m.e[i];
        if (t.key == key) {
            for (int g = begin; g < end; ++g) folds[g].t0 = t.t0[g - begin];
            *nsteps = t.nsteps;
            if (hit) *hit = true;
            return (int)i;
        }
    }
    int slot;
    if ((int)m.e.size() < SweepMemo::CAP) { slot = (int)m.e.size(); m.e.emplace_back(); }
    else { slot = m.next; m.next = (m.next + 1) % SweepMemo::CAP; }
    SweepTables& t = m.e[slot];
    t.key = key;
    sweep_schedule(folds, begin, end, &t.nsteps, nf, adopt);
    t.t0.clear();
    for (int g = begin; g < end; ++g) t.t0.push_back(folds[g].t0);
    t.tab.clear();
    sweep_flush_table(folds, begin, end, t.nsteps, wtot, 1 << 29, t.tab);
    t.n_gate = gate ? sweep_gate_table(folds, begin, end, t.nsteps, nf, t.tab) : -1;
    *nsteps = t.nsteps;
    if (hit) *hit = false;
    return slot;
}

// ---- a plan's root with the merge level that rides in its launch ------------------------------------------------------------
// One group triangle, by first slot: the root folds it at column 6 lo.
struct SweepTri {
    long long src;       // source offset (SweepFold::src_off)
    int lo, w;           // first clone slot, rows / columns
    int ld;              // row stride (SweepFold::ld)
    int prod;            // streamed root: 1 + the producer's progress word, 0: the triangle is there before the launch
};
// The merge nodes that ride: their folds are in the same list as the root's, and they are gated on the leaves or on nothing.
struct SweepRide { SweepNode* nodes; int count; int nf; bool gated; };
// What the root's launch reads of the host's tables, one instance per plan (the local plan, rank 0's merge plan).
struct RootTables {
    std::vector<int> image;   // [root flush | root gate | n offsets | node tables], the offsets counted from the end of the offset
                              // words; empty: the sweep is not in k_sweep form
    int n_gate = -1;          // step-0 requirements behind the root's flush + gate tables, -1: no gate table
    int merge_at = 0;         // where [n offsets | node tables] begins in the image
    bool streamed = false;    // the root's folds name their producers (SweepFold::prod), first fold not adopted
    int band = 0;             // widest row of the root block in columns
    void clear() { image.clear(); n_gate = -1; merge_at = 0; streamed = false; band = 0; }
};

// Appends the root's folds to `folds` and returns the root (envelopes and schedule set; out_off is the caller's).  In k_sweep
// form `out` gets the table image of the root and, streamed, of the riding nodes, whose schedules (and n_gate) are set again with
// `ride`'s slot count -- none adopted where they are gated.  Nodes with the same folds share one table.
inline SweepNode sweep_root(SweepMemo& memo, std::vector<SweepFold>& folds, const std::vector<SweepTri>& tris, int dc, bool k_sweep_form,
                            bool streamed, const SweepRide* ride, RootTables& out) {
    out.clear();
    out.streamed = streamed;
    SweepNode r{};
    r.fold_begin = (int)folds.size();
    int env = 0;
    for (const SweepTri& g : tris) {
        env = std::max(env, 6 * g.lo + g.w);
        SweepFold sf{}; sf.src_off = g.src; sf.off = 6 * g.lo; sf.w = g.w; sf.ew = env - 6 * g.lo; sf.ld = g.ld;
        if (streamed) sf.prod = g.prod;
        folds.push_back(sf);
        out.band = std::max(out.band, sf.ew);    // the root's rows become final one by one as the sweep passes them: K6-K7 follows
    }
    r.fold_end = (int)folds.size();
    r.wtot = dc;
    if (!k_sweep_form) { sweep_schedule(folds, r.fold_begin, r.fold_end, &r.nsteps, SWEEP_PLAN_NF, !streamed); return r; }
    // (the schedule comes with the flush table and, streamed, the gate table -- all three from the memo)
    const SweepTables& rt = memo.e[sweep_tables(memo, folds, r.fold_begin, r.fold_end, dc, SWEEP_PLAN_NF, !streamed, streamed, &r.nsteps)];
    out.image.assign(rt.tab.begin(), rt.tab.end());
    out.n_gate = rt.n_gate;
    if (!streamed || !ride) return r;
    // (one upload: the merge nodes' tables ride behind the root's; gated, each carries the node's gate table and step-0
    //  requirements behind its flush table)
    const size_t at0 = out.image.size(), n = (size_t)ride->count;
    out.merge_at = (int)at0;
    out.image.resize(at0 + n, 0);
    int at[SweepMemo::CAP];                       // where the memo's entry sits in this image, -1: not in it yet
    std::fill(at, at + SweepMemo::CAP, -1);
    for (size_t i = 0; i < n; ++i) {
        SweepNode& m = ride->nodes[i];
        bool hit = false;
        const int slot = sweep_tables(memo, folds, m.fold_begin, m.fold_end, m.wtot, ride->nf, !ride->gated, ride->gated, &m.nsteps, &hit);
        if (!hit) at[slot] = -1;                  // (the entry was written anew)
        if (at[slot] < 0) {
            at[slot] = (int)(out.image.size() - at0 - n);
            out.image.insert(out.image.end(), memo.e[slot].tab.begin(), memo.e[slot].tab.end());
        }
        out.image[at0 + i] = at[slot];
        m.n_gate = memo.e[slot].n_gate;
    }
    return r;
}

}  // namespace msckf
