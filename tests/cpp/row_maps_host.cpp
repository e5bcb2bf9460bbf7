// row_maps_host.cpp -- the LDS maps of the row-layout kernels (ukf_host.hpp: *_map) on the CPU (g++ under ASan / UBSan, compiled
// by tests/test_row_maps_host.py): the regions of every map are in ascending order and none overlaps the next, every aliased
// region lies inside the table it aliases, every slice is a multiple of four scalars, and the totals are the pinned ones.
#include <cstdio>
#include <initializer_list>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

struct Region {
    int at, size;   // offset from the map, size as the kernel uses the region
};

// the regions in slice order: the first starts the slice, none reaches into the next, the last ends inside PF; PF is a multiple of four
static void expect_ordered(const char* map, std::initializer_list<Region> regions, int PF) {
    int end = 0;
    bool first = true;
    for (const Region& r : regions) {
        if (first ? r.at != 0 : r.at < end) {
            std::printf("FAIL %s: region at %d starts before %d\n", map, r.at, end);
            ++failures;
        }
        first = false;
        EXPECT(r.size > 0);
        end = r.at + r.size;
    }
    if (end > PF || PF % 4 != 0) {
        std::printf("FAIL %s: PF %d, regions end at %d\n", map, PF, end);
        ++failures;
    }
}

// an aliased region lies inside its table
static void expect_inside(const char* map, Region alias, Region table) {
    if (alias.at < table.at || alias.size <= 0 || alias.at + alias.size > table.at + table.size) {
        std::printf("FAIL %s: alias [%d, %d) outside the table [%d, %d)\n", map, alias.at, alias.at + alias.size, table.at, table.at + table.size);
        ++failures;
    }
}

int main() {
    using namespace ukfb;
    struct { int S, D; } models[2] = {{13, 12}, {14, 13}};
    for (const auto& md : models) {
        const int S = md.S, D = md.D, N = 2 * D + 1, PK = D * (D + 1) / 2;
        // the sizes of the regions, written out: D columns or rows of stride 14, 16 pivots, the table of 2 D + 1 rows, a mean
        // padded to 16, a packed covariance padded to even, the rotation matrix, the sink
        const int cols = D * 14, piv = 16, table = N * 14, mean = 16, pke = (PK + 1) / 2 * 2, rot = 10, sink = 16;
        {
            const SmoothMap m = smooth_map(S, D);
            expect_ordered("smooth", {{m.FAC, cols}, {m.RSP, piv}, {m.TAB, table}, {m.CSM, mean}, {m.CSP, pke}, {m.MUF, mean}, {m.PKF, pke},
                                      {m.ROT, rot}, {m.DUM, sink}, {m.SMR, cols}, {m.MUP, mean}}, m.PF);
            expect_inside("smooth G", {m.GM, cols}, {m.TAB, table});
            expect_inside("smooth M", {m.MM, cols}, {m.TAB, table});
            EXPECT(m.GM + cols <= m.MM && m.LS == 14);
        }
        {
            const ForecastMap m = forecast_map(S, D);
            expect_ordered("forecast", {{m.FAC, cols}, {m.RSP, piv}, {m.TAB, table}, {m.CSM, mean}, {m.CSP, pke}, {m.ROT, rot}, {m.DUM, sink}}, m.PF);
            EXPECT(m.PF >= m.DUM + sink + FORECAST_SLICE_PAD && m.LS == 14);
        }
        {
            const StateMeasMap m = state_meas_map(S, D);
            expect_ordered("state", {{m.FAC, cols}, {m.RSP, piv}, {m.TAB, table}, {m.MUF, mean}, {m.PKF, pke}, {m.ZM, mean}, {m.PKQ, pke},
                                     {m.DUM, sink}}, m.PF);
            expect_inside("state Y", {m.YM, cols}, {m.TAB, table});
            EXPECT(m.LS == 14);
        }
        {
            const SensorMap m = sensor_map(S, D);
            expect_ordered("sensor", {{m.FAC, cols}, {m.RSP, piv}, {m.TAB, table}, {m.MUF, mean}, {m.PKF, pke}, {m.INP, 32}, {m.DUM, sink}}, m.PF);
            expect_inside("sensor W", {m.WT, D * m.ZS}, {m.TAB, table});
            expect_inside("sensor Y", {m.YM, D * m.ZS}, {m.TAB, table});
            EXPECT(m.WT + D * m.ZS <= m.YM && m.LS == 14 && m.ZS == 4 && SENSOR_INPUT_SCALARS <= 32);
        }
        {
            const SampledMap m = sampled_map(S, D);
            expect_ordered("sampled", {{m.FAC, cols}, {m.RSP, piv}, {m.TAB, table}, {m.MUF, mean}, {m.PKF, pke}, {m.INP, SAMPLED_INPUT_REGION},
                                       {m.DUM, sink}}, m.PF);
            expect_inside("sampled W", {m.WT, D * m.ZS}, {m.TAB, table});
            expect_inside("sampled Y", {m.YM, D * m.ZS}, {m.TAB, table});
            expect_inside("sampled staged", {m.ZST, N * SAMPLED_MAX_M}, {m.TAB, table});
            EXPECT(m.WT + D * m.ZS <= m.YM && m.YM + D * m.ZS <= m.ZST && m.LS == 14 && m.ZS == 6 && m.MM == 6);
        }
        {
            const SigmaPointsMap m = sigma_points_map(S, D);
            expect_ordered("sigma points", {{m.FAC, cols}, {m.RSP, piv}, {m.MUF, mean}, {m.PKF, pke}, {m.DUM, sink}}, m.PF);
            EXPECT(m.LS == 14);
        }
        {
            const PredictSampledMap m = predict_sampled_map(S, D);
            expect_ordered("predict-sampled", {{m.SMR, cols}, {m.TAB, table}, {m.CSM, mean}, {m.CSP, pke}, {m.DUM, sink}}, m.PF);
            expect_inside("predict-sampled staged", {m.STG, N * S}, {m.TAB, table});
            EXPECT(m.LS == 14);
        }
        {
            const ConditionMap m = condition_map(S, D);
            expect_ordered("condition", {{m.ROW, cols}, {m.VPB, cols}, {m.LAM, 16}, {m.SDV, 16}, {m.MUF, mean}, {m.PKF, pke}, {m.DUM, sink}}, m.PF);
            EXPECT(m.PF >= m.DUM + sink + CONDITION_SLICE_PAD && m.LS == 14);
        }
        {
            const DelayedMap m = delayed_map(S, D);
            const SmoothMap sm = smooth_map(S, D);
            expect_ordered("delayed", {{m.FAC, cols}, {m.RSP, piv}, {m.TAB, table}, {m.CSM, mean}, {m.CSP, pke}, {m.MUF, mean}, {m.PKF, pke},
                                       {m.ROT, rot}, {m.DUM, sink}, {m.SMR, cols}, {m.MUP, mean}, {m.MOP, cols}}, m.PF);
            expect_inside("delayed W", {m.WT, D * m.ZS}, {m.TAB, table});
            expect_inside("delayed Y_s", {m.YM, D * m.ZS}, {m.TAB, table});
            expect_inside("delayed Y_n", {m.YN, D * m.ZS}, {m.TAB, table});
            EXPECT(m.WT + D * m.ZS <= m.YM && m.YM + D * m.ZS <= m.YN && m.LS == 14 && m.ZS == 4);
            // the smoother's slice as it is, the operator behind it
            EXPECT(m.FAC == sm.FAC && m.RSP == sm.RSP && m.TAB == sm.TAB && m.GM == sm.GM && m.MM == sm.MM && m.CSM == sm.CSM && m.CSP == sm.CSP);
            EXPECT(m.MUF == sm.MUF && m.PKF == sm.PKF && m.ROT == sm.ROT && m.DUM == sm.DUM && m.SMR == sm.SMR && m.MUP == sm.MUP);
            EXPECT(m.MOP == sm.PF);
        }
    }
    // the totals the programs of the features pin
    EXPECT(smooth_map(13, 12).PF == 932 && smooth_map(14, 13).PF == 1016);
    EXPECT(forecast_map(13, 12).PF == 660 && forecast_map(14, 13).PF == 716);
    EXPECT(state_meas_map(13, 12).PF == 740 && state_meas_map(14, 13).PF == 808);
    EXPECT(sensor_map(13, 12).PF == 676 && sensor_map(14, 13).PF == 732);
    EXPECT(sampled_map(13, 12).PF == 740 && sampled_map(14, 13).PF == 796);
    EXPECT(sigma_points_map(13, 12).PF == 296 && sigma_points_map(14, 13).PF == 324);
    EXPECT(predict_sampled_map(13, 12).PF == 628 && predict_sampled_map(14, 13).PF == 684);
    EXPECT(condition_map(13, 12).PF == 484 && condition_map(14, 13).PF == 524);
    EXPECT(delayed_map(13, 12).PF == 1100 && delayed_map(14, 13).PF == 1200);
    // the size functions are the maps' totals, and refuse a filter that does not fit a row
    EXPECT(smooth_filter_scalars(13, 12) == 932 && forecast_filter_scalars(14, 13) == 716 && state_meas_filter_scalars(13, 12) == 740);
    EXPECT(sensor_filter_scalars(14, 13) == 732 && bearing_filter_scalars(13, 12) == 676 && sampled_filter_scalars(14, 13) == 796);
    EXPECT(sigma_points_filter_scalars(13, 12) == 296 && predict_sampled_filter_scalars(14, 13) == 684);
    EXPECT(condition_filter_scalars(13, 12) == 484 && delayed_filter_scalars(14, 13) == 1200);
    EXPECT(smooth_filter_scalars(17, 16) == -1 && forecast_filter_scalars(17, 16) == -1 && state_meas_filter_scalars(17, 16) == -1);
    EXPECT(sensor_filter_scalars(17, 16) == -1 && bearing_filter_scalars(17, 16) == -1 && sampled_filter_scalars(17, 16) == -1);
    EXPECT(sigma_points_filter_scalars(17, 16) == -1 && predict_sampled_filter_scalars(17, 16) == -1);
    EXPECT(condition_filter_scalars(17, 16) == -1 && delayed_filter_scalars(17, 16) == -1);
    return finish();
}
