// lifecycle_host.cpp -- the filter lifecycle's host decisions of ukf_host.hpp on the CPU (g++ under ASan / UBSan, compiled by
// tests/test_lifecycle_host.py): argument checks, launch geometry, the carving of the workspace.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

int main(int argc, char** argv) {
    using namespace ukfb;
    static_assert(LC_ROWS_PER_BLOCK == 16 && LC_COUNT_BLOCK == 1024 && LC_ROW == 16, "four records per wavefront, 1024 groups per count block");
    const int64_t big = 0x7fffffff;
    // (capacity, n, records, scatter, mu, cov, noise, noise_per_filter)
    EXPECT(check_lifecycle_args(1022, 257, true, false, false, false, false, false).rc == UKFB_OK);
    EXPECT(check_lifecycle_args(1022, 0, true, false, false, false, false, false).rc == UKFB_OK);
    EXPECT(check_lifecycle_args(1022, 5000, true, false, true, true, true, false).rc == UKFB_OK);    // gather: noise of a uniform engine is fine
    EXPECT(check_lifecycle_args(1022, big, true, true, true, true, false, false).rc == UKFB_OK);
    EXPECT(check_lifecycle_args(1022, 257, true, true, true, true, true, true).rc == UKFB_OK);
    EXPECT(check_lifecycle_args(big, 1, true, true, true, true, false, false).rc == UKFB_OK);
    EXPECT(check_lifecycle_args(1022, -1, true, false, false, false, false, false).rc == UKFB_ERR_OUT_OF_RANGE);
    EXPECT(check_lifecycle_args(1022, big + 1, true, true, true, true, false, false).rc == UKFB_ERR_OUT_OF_RANGE);
    EXPECT(check_lifecycle_args(big + 1, 1, true, true, true, true, false, false).rc == UKFB_ERR_OUT_OF_RANGE);
    EXPECT(check_lifecycle_args(1022, 257, false, false, false, false, false, false).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_lifecycle_args(1022, 257, true, true, false, true, false, false).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_lifecycle_args(1022, 257, true, true, true, false, false, false).rc == UKFB_ERR_INVALID_ARG);
    {   // noise records into batch-uniform storage: refused, and the text names the call that switches the storage
        const Verdict v = check_lifecycle_args(1022, 257, true, true, true, true, true, false);
        EXPECT(v.rc == UKFB_ERR_INVALID_ARG && v.msg && std::string(v.msg).find("ukfb_set_process_noise_per_filter") != std::string::npos);
    }
    EXPECT(check_lifecycle_args(1022, -1, false, true, false, false, true, false).msg != nullptr);
    // compact: every group size, the refusals
    for (int group = 1; group <= 8; ++group) {
        EXPECT(check_compact_args(840, group).rc == UKFB_OK);   // 840 = lcm(1 ... 8)
        EXPECT(check_compact_args(841, group).rc == (group == 1 ? UKFB_OK : (841 % group ? UKFB_ERR_INVALID_ARG : UKFB_OK)));
    }
    EXPECT(check_compact_args(840, 0).rc == UKFB_ERR_INVALID_ARG && check_compact_args(840, 9).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_compact_args(840, -1).rc == UKFB_ERR_INVALID_ARG && check_compact_args(5, 3).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_compact_args(big + 1, 1).rc == UKFB_ERR_OUT_OF_RANGE && check_compact_args(big, 1).rc == UKFB_OK);
    EXPECT(check_compact_args(5, 3).msg != nullptr && check_compact_args(5, 0).msg != nullptr);
    // record and item grids
    EXPECT(lifecycle_record_blocks(1) == 1 && lifecycle_record_blocks(16) == 1 && lifecycle_record_blocks(17) == 2);
    EXPECT(lifecycle_record_blocks(257) == 17 && lifecycle_record_blocks(big) == (big + 15) / 16 && lifecycle_record_blocks(big) <= 0x7fffffff);
    EXPECT(lifecycle_item_blocks(1) == 1 && lifecycle_item_blocks(256) == 1 && lifecycle_item_blocks(257) == 2);
    // geometry over capacities and groups: the pieces of the workspace are disjoint, aligned and large enough for every group
    const int64_t caps[] = {1, 3, 4, 5, 40003, 40000000};
    for (const int64_t cap : caps) {
        const LifecycleGeometry one = lifecycle_geometry(cap, 1);
        for (int group = 1; group <= 8; ++group) {
            if (check_compact_args(cap, group).rc != UKFB_OK) continue;
            const LifecycleGeometry g = lifecycle_geometry(cap, group);
            EXPECT(g.groups * group == cap);
            EXPECT(int64_t(g.count_blocks) * LC_COUNT_BLOCK >= g.groups && int64_t(g.count_blocks - 1) * LC_COUNT_BLOCK < g.groups);
            EXPECT(g.count_blocks >= 1 && g.move_blocks >= 1 && g.move_blocks <= LC_MOVE_MAX_BLOCKS);
            EXPECT(2 * (g.pair_cap - 1) <= g.groups && 2 * g.pair_cap > g.groups);   // min(L, G - L) <= G / 2 < pair_cap
            EXPECT(g.ws_words == one.ws_words && g.owner_off == one.owner_off && g.mover_off == one.mover_off);   // one workspace serves every group
            const size_t offs[] = {g.owner_off, g.counts_off, g.before_off, g.totals_off, g.hole_off, g.mover_off, g.ws_words};
            const size_t need[] = {size_t(cap), size_t(g.count_blocks), size_t(g.count_blocks), 4, size_t(g.pair_cap), size_t(g.pair_cap)};
            for (int p = 0; p < 6; ++p) EXPECT(offs[p] % 64 == 0 && offs[p] + need[p] <= offs[p + 1]);
        }
        EXPECT(one.owner_off == 0 && one.ws_words * 4 <= size_t(cap) * 8 + size_t(cap) / 128 + 8 * 256);   // two words a filter, the counts, the alignment
    }
    EXPECT(lifecycle_geometry(1, 1).move_blocks == 1 && lifecycle_geometry(3, 3).groups == 1);
    EXPECT(lifecycle_geometry(40003, 1).count_blocks == 40 && lifecycle_geometry(40003, 1).move_blocks == 1251);
    EXPECT(lifecycle_geometry(40000000, 1).count_blocks == 39063 && lifecycle_geometry(40000000, 1).move_blocks == LC_MOVE_MAX_BLOCKS);
    EXPECT(lifecycle_geometry(40000000, 8).groups == 5000000 && lifecycle_geometry(40000000, 8).count_blocks == 4883);
    // the N of the GPU compact test (argv[1]): at least three count blocks for every group it uses, the last one ragged
    if (argc > 1) {
        const int64_t n = std::atoll(argv[1]);
        for (const int group : {1, 3, 8}) {
            const LifecycleGeometry g = lifecycle_geometry(n / group * group, group);
            EXPECT(g.count_blocks >= 3 && g.groups % LC_COUNT_BLOCK != 0);
        }
    }
    return finish();
}
