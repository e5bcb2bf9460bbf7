// smooth_host.cpp -- the smoother's host decisions of ukf_host.hpp on the CPU (g++ under ASan / UBSan, compiled by
// tests/test_smooth_host.py): argument checks, the chunking of a window into launches, the LDS byte count.
#include <cstdio>
#include <vector>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

int main() {
    using namespace ukfb;
    // steps against slots, first_slot range, NULL rings
    EXPECT(check_smooth_args(2, 2, 0, true, true, true, true).rc == UKFB_OK);
    EXPECT(check_smooth_args(6, 8, 5, true, true, true, true).rc == UKFB_OK);
    EXPECT(check_smooth_args(1, 8, 0, true, true, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_smooth_args(0, 8, 0, true, true, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_smooth_args(9, 8, 0, true, true, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_smooth_args(2, 0, 0, true, true, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_smooth_args(4, 8, 8, true, true, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_smooth_args(4, 8, -1, true, true, true, true).rc == UKFB_ERR_INVALID_ARG);
    for (int k = 0; k < 4; ++k) {
        const Verdict v = check_smooth_args(4, 8, 0, k != 0, k != 1, k != 2, k != 3);
        EXPECT(v.rc == UKFB_ERR_INVALID_ARG && v.msg != nullptr);
    }
    EXPECT(check_history_args(8, 7, true, true).rc == UKFB_OK);
    EXPECT(check_history_args(8, 8, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_history_args(8, -1, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_history_args(0, 0, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_history_args(8, 0, false, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_history_args(8, 0, true, false).rc == UKFB_ERR_INVALID_ARG);
    // chunking: at most 32 backward steps per launch, every backward step exactly once, the slots across a ring wrap
    const int expect_launches[4][2] = {{2, 1}, {33, 1}, {34, 2}, {65, 2}};
    for (const auto& el : expect_launches) {
        const int steps = el[0], slots = steps + 3, first = slots - 2;   // the window wraps after two steps
        const SmoothPlan plan(steps, slots, first);
        EXPECT(plan.launches() == el[1]);
        std::vector<int> written(size_t(steps), 0);
        int top = steps - 1;
        for (int k = 0; k < plan.launches(); ++k) {
            const SmoothLaunch L = plan[k];
            EXPECT(L.first == (k == 0));
            EXPECT(L.top_step == top);                       // starts from what the launch before stored last
            EXPECT(L.top_slot == (first + L.top_step) % slots);
            EXPECT(L.back >= 1 && L.back <= SMOOTH_MAX_BACK);
            EXPECT(L.dt_first == L.top_step - 1);
            for (int j = 0; j < L.back; ++j) {
                const int c = L.top_step - 1 - j;
                EXPECT(c >= 0 && L.dt_first - j == c);       // step c redoes the prediction of dt[c]
                if (c >= 0) ++written[size_t(c)];
            }
            top = L.top_step - L.back;
        }
        EXPECT(top == 0);
        for (int c = 0; c + 1 < steps; ++c) EXPECT(written[size_t(c)] == 1);
        EXPECT(written[size_t(steps - 1)] == 0);
    }
    EXPECT(SmoothPlan(34, 40, 0)[0].back == 32 && SmoothPlan(34, 40, 0)[1].back == 1 && SmoothPlan(34, 40, 0)[1].top_step == 1);
    EXPECT(SmoothPlan(65, 65, 64)[1].top_slot == (64 + 32) % 65);
    // LDS per model and precision: four filters per workgroup
    struct { int S, D; } models[2] = {{13, 12}, {14, 13}};
    for (const auto& m : models) {
        const int PK = m.D * (m.D + 1) / 2;
        const int sc = smooth_filter_scalars(m.S, m.D);
        // two D x 14 matrices and the delta table, two records, and no more than 15 % on top
        const int floor_sc = 2 * m.D * ROW_LS + (2 * m.D + 1) * ROW_LS + 2 * (m.S + PK);
        EXPECT(sc >= floor_sc && sc <= floor_sc * 115 / 100 && sc % 2 == 0);
        for (size_t bytes : {size_t(4), size_t(8)}) {
            const RowGeometry g = smooth_geometry(m.S, m.D, 1022, bytes);
            EXPECT(g.grid == 256 && g.lds_bytes == int(4 * sc * bytes));
            EXPECT(g.lds_bytes <= 65536 && g.lds_bytes % 16 == 0);
            EXPECT((sc * int(bytes) / 4) % 32 != 0);   // the four slices start on different banks
        }
        EXPECT(smooth_geometry(m.S, m.D, 0, 8).grid == 0 && smooth_geometry(m.S, m.D, 5, 8).grid == 2);
    }
    EXPECT(smooth_filter_scalars(13, 12) == 932 && smooth_filter_scalars(14, 13) == 1016);
    // the shape tests/test_gpu_smooth.py pushes behind: 16 384 filters on an engine with a second stream run as split launches
    EXPECT(split_launch(false, false, true, true, 16384, 262144) && SPLIT_MIN_FILTERS <= 16384);
    EXPECT(!split_launch(false, false, false, true, 16384, 262144) && !split_launch(false, false, true, false, 16384, 262144));
    return finish();
}
