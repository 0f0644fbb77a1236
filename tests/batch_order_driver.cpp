// Text driver of csrc/batch_order.h for tests/test_batch_order.py: built with the host compiler from the header alone.
// One batch per input line:
//   batch N maxM split direct_cap wide_window rem_rows_cap rec_cap nch F view_ptr[F + 1] obs_slot[view_ptr[F]]
// (rem_rows_cap < 0: no split records; rec_cap < 0: the raw layout's; nch: the ranges the scan is cut into, as the host pool
// cuts it).  Per batch it prints the scan's code, the keys, what build() returned, the BatchOrder as it stands afterwards -- one
// value lives through the whole script, as in a context --, and after a success the records and both layouts; then `end`.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "batch_order.h"

using namespace msckf;

template <class V>
static void line(const char* name, const V& v) {
    std::printf("%s", name);
    for (const auto& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

static void print_order(const BatchOrder& o) {
    if (!o.valid) { std::printf("order invalid\n"); return; }
    std::printf("order Fb %d Fw %d Fs %d nNarrow %d sumMs %d split_on %d rem_cap %d Mmax %d %d %d stack %lld\n", o.Fb, o.Fw, o.Fs,
                o.nNarrow, o.sumMs, (int)o.split_on, o.rem_cap, o.Mmax, o.Mmax_band, o.Mmax_wide, o.stack_elems);
    line("perm", o.perm); line("view", o.h_view); line("fmin", o.h_fmin); line("fmax", o.h_fmax); line("parent", o.h_parent);
    for (const SplitRec& s : o.h_split) {
        std::printf("split");
        for (int g = 0; g < SPLIT_MAXG; ++g) std::printf(" %d", s.child[g]);
        std::printf(" wide %d gv", s.wide);
        for (int g = 0; g <= SPLIT_MAXG; ++g) std::printf(" %d", (int)s.gv[g]);
        std::printf(" ng %d rows %d\n", (int)s.ng, s.rows_cap);
    }
}

int main() {
    BatchOrder order;
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string word;
        int N, maxM, split, direct_cap, wide_window, rem_rows_cap, nch, F;
        long long rec_cap;
        in >> word >> N >> maxM >> split >> direct_cap >> wide_window >> rem_rows_cap >> rec_cap >> nch >> F;
        if (!in || word != "batch" || F < 1 || nch < 1) { std::printf("bad line\n"); return 2; }
        std::vector<int32_t> view_ptr(F + 1);
        for (int& x : view_ptr) in >> x;
        std::vector<int32_t> obs_slot(view_ptr[F] > 0 ? view_ptr[F] : 0);
        for (int& x : obs_slot) in >> x;
        if (!in) { std::printf("bad line\n"); return 2; }
        // the scan, range by range; the lowest failing range decides
        std::vector<int> key_in(F);
        std::vector<unsigned char> M_in(F);
        ScanPart tot;
        int rc = kOrderOk;
        for (int ch = 0; ch < nch && rc == kOrderOk; ++ch) {
            const int f0 = (int)((long long)F * ch / nch), f1 = (int)((long long)F * (ch + 1) / nch);
            const ScanPart part = scan_range(N, maxM, split != 0, view_ptr.data(), obs_slot.data(), f0, f1, key_in.data(), M_in.data());
            rc = part.err;
            tot.add(part);
        }
        std::printf("rc %d\n", rc);
        if (rc == kOrderOk) {
            const bool keep = tot.Mmax[2] > 0 && rem_rows_cap < 0 && keeps_wide_tiles(tot.n_mid, tot.n_long, F, direct_cap, wide_window != 0);
            if (keep) drop_split_class(N, F, key_in.data(), tot);
            std::printf("scan Mmax %d %d %d mid %d long %d keep %d\n", tot.Mmax[0], tot.Mmax[1], tot.Mmax[2], tot.n_mid, tot.n_long, (int)keep);
            line("key", key_in);
            const RawLayout raw = raw_layout(F, view_ptr[F]);
            std::vector<GatherRec> rec(raw.rec_cap);
            const BatchOrder::Fail fail = order.build(N, F, view_ptr.data(), obs_slot.data(), key_in.data(), M_in.data(), tot,
                                                      rec_cap < 0 ? raw.rec_cap : (size_t)rec_cap, rem_rows_cap, rec.data());
            std::printf("build %d\n", (int)fail);
            print_order(order);
            if (fail == BatchOrder::kBuilt) {
                std::printf("rec");
                for (int e = 0; e < order.Fs; ++e) std::printf(" %d %d %d %d %lld", rec[e].f, rec[e].a, rec[e].M, rec[e].o, rec[e].blk);
                std::printf("\n");
                std::printf("raw %zu %zu %zu %zu %zu bytes %zu rec_cap %zu pin %zu split_off %zu\n", raw.r_uv, raw.r_base, raw.r_m, raw.r_rho,
                            raw.r_slot, raw.raw_bytes, raw.rec_cap, raw.pin_bytes, raw.split_off(order.Fs));
                const SortedLayout so = sorted_layout(order.Fs, order.sumMs, 32);
                std::printf("sorted %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu bytes %zu\n", so.o_uv, so.o_base, so.o_m, so.o_rho, so.o_blk,
                            so.o_view, so.o_perm, so.o_slot, so.o_fmin, so.o_info, so.feat_bytes);
            }
        } else {
            print_order(order);           // (the scan touches no BatchOrder: the last good batch's, unchanged)
        }
        std::printf("end\n");
    }
    return 0;
}
