// Drives csrc/track_mirror.h from a script on stdin (tests/test_track_mirror.py; tests/track_mirror_model.py is the model the
// output is compared with).  One operation per line:
//   size T V | clear | observe NEWEST n id.. | frame NEWEST WITH_DESC n (id uv_finite result).. | remove n id..
//   drop N mask[N] | rows | created | where N want[N]
// After each: "rc <code> bad <pair or -1>", for an enumeration "rows <row>..", then the whole mirror:
//   tracks <n> views <n> | free <row>.. | dropped <id>..
//   id <id> row <r> anchor <a> lost <l> tracked <t> rank <creation rank> desc <0|1> slots <s>..   (ascending id)
//   end
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "track_mirror.h"

static void dump(const TrackMirror& m) {
    std::printf("tracks %d views %lld | free", m.n_tracks(), m.n_views());
    for (int r : m.free_rows()) std::printf(" %d", r);
    std::printf(" | dropped");
    for (int id : m.dropped()) std::printf(" %d", id);
    std::printf("\n");
    std::vector<int> by_creation, rank(m.rows(), -1);
    m.live_rows_by_creation(by_creation);
    for (size_t k = 0; k < by_creation.size(); ++k) rank[by_creation[k]] = (int)k;
    std::vector<std::pair<int, int>> live;                           // (id, row)
    for (int r : by_creation) live.emplace_back(m.id(r), r);
    std::sort(live.begin(), live.end());
    for (const auto& e : live) {
        const int r = e.second;
        if (m.row_of(e.first) != r) std::printf("row_of(%d) = %d !\n", e.first, m.row_of(e.first));
        std::printf("id %d row %d anchor %d lost %d tracked %d rank %d desc %d slots", e.first, r, m.anchor(r), m.lost(r),
                    m.tracked(r), rank[r], (int)m.hasdesc(r));
        for (int v = 0; v < m.M(r); ++v) std::printf(" %d", m.slots(r)[v]);
        std::printf("\n");
    }
    std::printf("end\n");
}

int main() {
    TrackMirror m;
    std::string op;
    while (std::cin >> op) {
        int rc = 0, bad = -1;
        std::vector<int> rows;
        bool listing = false;
        if (op == "size") {
            int T, V;
            std::cin >> T >> V;
            m.size(T, V);
        } else if (op == "clear") {
            m.clear();
        } else if (op == "observe" || op == "frame") {
            const bool frame = op == "frame";
            int newest, with_desc = 0, n;
            std::cin >> newest;
            if (frame) std::cin >> with_desc;
            std::cin >> n;
            std::vector<int32_t> ids(n);
            std::vector<int> finite(n, 1), res(n, 0);
            for (int i = 0; i < n; ++i) {
                std::cin >> ids[i];
                if (frame) std::cin >> finite[i] >> res[i];
            }
            std::vector<TrackPlace> place(n);
            rc = frame ? m.plan(ids.data(), n, newest, place.data(), &bad, [&](int i) { return finite[i] != 0; })
                       : m.plan(ids.data(), n, newest, place.data(), &bad);
            if (rc == 0) {
                for (int i = 0; i < n; ++i)
                    m.commit(ids[i], place[i], newest, !frame || (res[i] != 1 && res[i] != 2), frame && with_desc);
                if (frame) m.age_unlisted(place.data(), n);
            }
        } else if (op == "remove") {
            int n;
            std::cin >> n;
            std::vector<int32_t> ids(n);
            for (int& id : ids) std::cin >> id;
            rc = m.remove(ids.data(), n);
        } else if (op == "drop") {
            int N;
            std::cin >> N;
            std::vector<short> remap(N);
            for (int s = 0, k = 0; s < N; ++s) {
                int gone;
                std::cin >> gone;
                remap[s] = gone ? (short)-1 : (short)k++;
            }
            m.drop_clones(remap.data());
        } else if (op == "rows") {
            m.live_rows(rows); listing = true;
        } else if (op == "created") {
            m.live_rows_by_creation(rows); listing = true;
        } else if (op == "where") {
            int N;
            std::cin >> N;
            std::vector<char> want(N);
            for (int s = 0; s < N; ++s) { int w; std::cin >> w; want[s] = (char)w; }
            m.live_rows_by_creation(want, rows); listing = true;
        } else {
            std::fprintf(stderr, "unknown operation %s\n", op.c_str());
            return 2;
        }
        std::printf("rc %d bad %d\n", rc, bad);
        if (listing) {
            std::printf("rows");
            for (int r : rows) std::printf(" %d", r);
            std::printf("\n");
        }
        dump(m);
    }
    return 0;
}
