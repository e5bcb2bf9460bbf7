// delayed_host.cpp -- the host decisions of the delayed-measurement update (ukf_host.hpp) on the CPU (g++ under ASan / UBSan,
// compiled by tests/test_delayed_host.py): argument checks, the steps / slots limits, the LDS byte count, the lag rule.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

// the rule as include/ukf_batch.h words it, written independently of delayed_lag_of
static int lag_by_the_words(const std::vector<int64_t>& ts, int64_t t) {
    const int steps = int(ts.size()), n = steps - 1;
    if (t >= ts[size_t(n)]) return 0;
    if (t < ts[0] && steps > 1 && 2 * (ts[0] - t) > ts[1] - ts[0]) return steps;
    if (t < ts[0] && steps == 1) return steps;
    int best = 0;
    for (int c = 1; c < steps; ++c)
        if (std::llabs(ts[size_t(c)] - t) < std::llabs(ts[size_t(best)] - t)) best = c;
    return n - best;
}

int main() {
    using namespace ukfb;
    double dt[40] = {};
    char ring = 0;
    ukfb_delayed_in in{};
    in.steps = 6; in.dt = dt; in.slots = 8; in.first_slot = 5;
    in.mu_hist_dev = &ring; in.cov_hist_dev = &ring; in.z_dev = &ring; in.Q_dev = &ring;
    ukfb_delayed_out out{};
    out.mu_out = &ring;
    EXPECT(check_delayed_args(&in, 1, nullptr).rc == UKFB_OK);          // commit = 1 needs no output
    EXPECT(check_delayed_args(&in, 0, &out).rc == UKFB_OK);
    EXPECT(check_delayed_args(&in, 0, nullptr).rc == UKFB_ERR_INVALID_ARG);
    ukfb_delayed_out none{};
    EXPECT(check_delayed_args(&in, 0, &none).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_delayed_args(nullptr, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_delayed_args(&in, 2, &out).rc == UKFB_ERR_INVALID_ARG);
    {   // every required pointer, one at a time
        const void** req[4] = {&in.mu_hist_dev, &in.cov_hist_dev, &in.z_dev, &in.Q_dev};
        for (auto p : req) {
            const void* keep = *p;
            *p = nullptr;
            const Verdict v = check_delayed_args(&in, 1, nullptr);
            EXPECT(v.rc == UKFB_ERR_INVALID_ARG && v.msg != nullptr);
            *p = keep;
        }
    }
    {   // steps / slots / first_slot
        ukfb_delayed_in a = in;
        a.steps = 1; a.dt = nullptr;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_OK);       // a window of the present alone: lag 0 only
        a.steps = 2;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);   // dt missing
        a = in; a.steps = 0;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        a = in; a.steps = 9;                                             // more steps than slots
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_OUT_OF_RANGE);
        a = in; a.slots = 64; a.steps = DELAYED_MAX_STEPS;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_OK);
        a.steps = DELAYED_MAX_STEPS + 1;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_OUT_OF_RANGE);
        a = in; a.first_slot = 8;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        a.first_slot = -1;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        a = in; a.slots = 0;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        a = in; a.q_is_uniform = 2;
        EXPECT(check_delayed_args(&a, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
    }
    EXPECT(DELAYED_MAX_STEPS == 33 && DELAYED_MAX_STEPS - 1 == SMOOTH_MAX_BACK);
    // LDS: the smoother's slice and D rows of M behind it, a multiple of four scalars; four filters of either model fit the
    // 160 KiB of a compute unit at least four times in fp64
    for (const int* sd : {(const int[]){13, 12}, (const int[]){14, 13}}) {
        const int S = sd[0], D = sd[1], pf = delayed_filter_scalars(S, D);
        EXPECT(pf % 4 == 0 && pf >= smooth_filter_scalars(S, D) + D * ROW_LS && pf < smooth_filter_scalars(S, D) + D * ROW_LS + 4);
        const RowGeometry g8 = delayed_geometry(S, D, 1022, 8), g4 = delayed_geometry(S, D, 1022, 4);
        EXPECT(g8.grid == 256 && g4.grid == 256);
        EXPECT(g8.lds_bytes == 4 * pf * 8 && g4.lds_bytes == 4 * pf * 4);
        EXPECT(4 * g8.lds_bytes <= 160 * 1024);
        EXPECT(delayed_geometry(S, D, 0, 8).grid == 0 && delayed_geometry(S, D, 1, 8).grid == 1 && delayed_geometry(S, D, 5, 8).grid == 2);
    }
    EXPECT(delayed_filter_scalars(13, 12) == 1100 && delayed_filter_scalars(14, 13) == 1200);
    EXPECT(delayed_filter_scalars(17, 16) == -1);
    // the lag helper's arguments and its rule
    const std::vector<int64_t> ts = {1000, 2000, 3100, 4000, 5000};
    EXPECT(check_delayed_lag_args(5, ts.data(), true, true).rc == UKFB_OK);
    EXPECT(check_delayed_lag_args(0, ts.data(), true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_delayed_lag_args(5, nullptr, true, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_delayed_lag_args(5, ts.data(), false, true).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_delayed_lag_args(5, ts.data(), true, false).rc == UKFB_ERR_INVALID_ARG);
    {
        std::vector<int64_t> many(40);
        for (size_t i = 0; i < many.size(); ++i) many[i] = int64_t(i) * 10;
        EXPECT(check_delayed_lag_args(33, many.data(), true, true).rc == UKFB_OK);
        EXPECT(check_delayed_lag_args(34, many.data(), true, true).rc == UKFB_ERR_OUT_OF_RANGE);
        many[7] = many[6];
        EXPECT(check_delayed_lag_args(33, many.data(), true, true).rc == UKFB_ERR_INVALID_ARG);   // not strictly increasing
    }
    const int64_t t[13] = {5000, 9000, 4999, 4500, 4501, 3550, 1000, 600, 500, 499, -7000, 2550, 1500};
    const int want[13] = {0, 0, 0, 1, 0, 2, 4, 4, 4, 5, 5, 3, 4};   // ties go to the older step; 500 is the edge, 499 is out
    for (int i = 0; i < 13; ++i) EXPECT(delayed_lag_of(5, ts.data(), t[i]) == want[i]);
    for (int64_t x = -1500; x <= 6500; x += 7) EXPECT(delayed_lag_of(5, ts.data(), x) == lag_by_the_words(ts, x));
    const std::vector<int64_t> one = {1000};
    EXPECT(delayed_lag_of(1, one.data(), 1000) == 0 && delayed_lag_of(1, one.data(), 2000) == 0 && delayed_lag_of(1, one.data(), 999) == 1);
    return finish();
}
