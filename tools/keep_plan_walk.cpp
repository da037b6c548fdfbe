// Stand-alone walk of the "keep_phase1" admission rule (dvt_circuits_amd/csrc/keep_plan.h) over the long jobs of DESIGN.md
// section 8, for a sanitizer build of the header on the host:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dvt_circuits_amd/csrc tools/keep_plan_walk.cpp -o keep_plan_walk
// The model: 280 of 288 GB free at the start, 24 GB reserved; a shard keeps 2.95 GB in full, 0.268 GB as a tree and uploads
// 0.10 GB; when shard i is admitted the fast pass has found min(S, 4 i + 9) shards.  Exit code 0 when the tier counts are
// those of the table (tests/test_keep_plan.py walks the same jobs through the library).
#include <cstdio>
#include <initializer_list>

#include "keep_plan.h"

int main() {
    using namespace dvt;
    const uint64_t GB = 1000000000ull, F = 2950000000ull, T = 268000000ull, UP = 100000000ull;
    const struct { uint64_t shards, full, tree; } want[] = {{32, 32, 0}, {90, 83, 7}, {128, 77, 51}, {256, 60, 196}, {384, 42, 342}, {511, 25, 486}};
    int bad = 0;
    for (auto &w : want) {
        uint64_t free_b = 280 * GB, count[3] = {0, 0, 0};
        for (uint64_t i = 0; i < w.shards; i++) {
            free_b -= UP;
            const uint64_t found = 4 * i + 9 < w.shards ? 4 * i + 9 : w.shards;
            KeepPlanIn in;
            in.mode = 2;
            in.free_b = free_b; in.total_b = 288 * GB; in.reserve = 24 * GB;
            in.full_b = F; in.tree_b = T; in.later_b = T + UP;
            in.remaining = found - i - 1; in.count_known = found == w.shards;
            in.full_kept = count[KEEP_FULL];
            const int tier = keep_plan(in);
            count[tier]++;
            free_b -= tier == KEEP_FULL ? F : tier == KEEP_TREE ? T : 0;
        }
        const bool ok = count[KEEP_FULL] == w.full && count[KEEP_TREE] == w.tree && count[KEEP_NONE] == 0;
        printf("%3llu shards: %llu full, %llu tree, %llu none%s\n", (unsigned long long)w.shards, (unsigned long long)count[KEEP_FULL],
               (unsigned long long)count[KEEP_TREE], (unsigned long long)count[KEEP_NONE], ok ? "" : "  <- not the table's");
        bad += !ok;
    }
    // the edges: sums that leave 64 bits, every mode, caps on either side
    for (int mode = -1; mode <= 3; mode++)
        for (uint64_t v : {(uint64_t)0, (uint64_t)1, 24 * GB, ~(uint64_t)0 - 1, ~(uint64_t)0})
            for (int64_t cap : {(int64_t)-1, (int64_t)0, (int64_t)1}) {
                KeepPlanIn in;
                in.mode = mode; in.free_b = v; in.total_b = ~0ull; in.reserve = v / 2; in.full_b = v; in.tree_b = v / 3; in.later_b = v;
                in.remaining = v; in.count_known = (v & 1) != 0; in.full_cap = cap; in.full_kept = v;
                const int tier = keep_plan(in);
                bad += tier < KEEP_NONE || tier > KEEP_FULL;
            }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
