// Drives csrc/sweep_plan.h from a script on stdin (tests/test_sweep_plan.py; tests/sweep_plan_model.py is the model the output
// is compared with).  Numbers separated by white space:
//   node WTOT NF ADOPT GATE RC K, then K folds OFF W EW PROD LD
//     t0 <t0 of every fold> | nsteps <n>                      sweep_schedule(NF, ADOPT)
//     flush <ring verdict 0|1> <nsteps + 1 entries>           sweep_flush_table(rc = RC)
//     gate <step-0 count> <nsteps + 2 entries, step-0 list>   sweep_gate_table(NF)
//     publish <nsteps + 1 entries>                            sweep_publish_table behind the flush entries
//     memo <slot> <hit 0|1> | tables <nsteps> <n_gate> <t0 ..> : <table ..>     sweep_tables(GATE) and the memo's entry
//   clear                                                     the memo forgets everything
//   root DC FORM STREAMED NTRI NRIDE RIDE_NF GATED, then NTRI triangles LO W LD PROD, then NRIDE nodes: WTOT K and K folds
//     root <fold_begin> <fold_end> <wtot> <nsteps> band <b> n_gate <n> merge_at <a> streamed <s>
//     fold <off> <w> <ew> <t0> <prod> <ld>   per root fold | ride <nsteps> <n_gate> <t0 ..>   per riding node | image <words>
// Every block closes with "end".
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sweep_plan.h"

using namespace msckf;

static void line(const char* name, const std::vector<int>& v, size_t from = 0) {
    std::printf("%s", name);
    for (size_t i = from; i < v.size(); ++i) std::printf(" %d", v[i]);
    std::printf("\n");
}

static void read_folds(std::vector<SweepFold>& folds, int k) {
    for (int i = 0; i < k; ++i) {
        SweepFold f{};
        std::cin >> f.off >> f.w >> f.ew >> f.prod >> f.ld;
        f.t0 = -1;
        folds.push_back(f);
    }
}

int main() {
    SweepMemo memo;
    std::string op;
    while (std::cin >> op) {
        if (op == "node") {
            int wtot, nf, adopt, gate, rc, k;
            std::cin >> wtot >> nf >> adopt >> gate >> rc >> k;
            std::vector<SweepFold> folds(3);                  // (the node's folds do not begin the list)
            const int b = (int)folds.size();
            read_folds(folds, k);
            const int e = (int)folds.size();
            int nsteps = -1;
            sweep_schedule(folds, b, e, &nsteps, nf, adopt != 0);
            std::vector<int> t0, tab{7, 7};                   // (nor does its table)
            for (int g = b; g < e; ++g) t0.push_back(folds[g].t0);
            line("t0", t0);
            std::printf("nsteps %d\n", nsteps);
            const bool ok = sweep_flush_table(folds, b, e, nsteps, wtot, rc, tab);
            std::printf("flush %d", (int)ok);
            line("", tab, 2);
            std::vector<int> gt{7};
            const int n0 = sweep_gate_table(folds, b, e, nsteps, nf, gt);
            std::printf("gate %d", n0);
            line("", gt, 1);
            sweep_publish_table(tab, 2, nsteps, wtot);
            line("publish", tab, 2 + nsteps + 1);
            for (int g = b; g < e; ++g) folds[g].t0 = -1;
            bool hit = false;
            int ns2 = -1;
            const int slot = sweep_tables(memo, folds, b, e, wtot, nf, adopt != 0, gate != 0, &ns2, &hit);
            std::printf("memo %d %d\n", slot, (int)hit);
            const SweepTables& t = memo.e[slot];
            std::printf("tables %d %d", ns2, t.n_gate);
            for (int g = b; g < e; ++g) std::printf(" %d", folds[g].t0);
            if (t.nsteps != ns2 || (int)t.t0.size() != k) std::printf(" entry!");
            line(" :", t.tab);
        } else if (op == "clear") {
            memo.e.clear();
        } else if (op == "root") {
            int dc, form, streamed, ntri, nride, ride_nf, gated;
            std::cin >> dc >> form >> streamed >> ntri >> nride >> ride_nf >> gated;
            std::vector<SweepTri> tris(ntri);
            for (SweepTri& t : tris) { t.src = 0; std::cin >> t.lo >> t.w >> t.ld >> t.prod; }
            std::vector<SweepFold> folds;
            std::vector<SweepNode> nodes;
            for (int i = 0; i < nride; ++i) {
                SweepNode m{};
                int k;
                std::cin >> m.wtot >> k;
                m.fold_begin = (int)folds.size();
                read_folds(folds, k);
                m.fold_end = (int)folds.size();
                m.nsteps = -1;
                nodes.push_back(m);
            }
            SweepRide ride{nodes.data(), nride, ride_nf, gated != 0};
            RootTables out;
            out.image.assign(5, 9);                           // (what an earlier plan left)
            const SweepNode r = sweep_root(memo, folds, tris, dc, form != 0, streamed != 0, nride ? &ride : nullptr, out);
            std::printf("root %d %d %d %d band %d n_gate %d merge_at %d streamed %d\n", r.fold_begin, r.fold_end, r.wtot, r.nsteps,
                        out.band, out.n_gate, out.merge_at, (int)out.streamed);
            for (int g = r.fold_begin; g < r.fold_end; ++g)
                std::printf("fold %d %d %d %d %d %d\n", folds[g].off, folds[g].w, folds[g].ew, folds[g].t0, folds[g].prod, folds[g].ld);
            for (const SweepNode& m : nodes) {
                std::printf("ride %d %d", m.nsteps, m.n_gate);
                for (int g = m.fold_begin; g < m.fold_end; ++g) std::printf(" %d", folds[g].t0);
                std::printf("\n");
            }
            line("image", out.image);
        } else {
            std::fprintf(stderr, "unknown operation %s\n", op.c_str());
            return 2;
        }
        std::printf("end\n");
    }
    return 0;
}
