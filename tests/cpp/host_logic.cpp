// host_logic.cpp -- the engine's host decisions (slam-pose_estimation_amd/csrc/ukf_host.hpp) on the CPU, built with g++ under
// ASan / UBSan (make host_asan; run by tests/test_host_logic.py).  Argument: a file of process-noise cases written by that test
// from synth.py, one per line: name model D expected(0/1) then D*D values.  Prints one line per failed check, exits 1 if any.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

namespace {
// EXPECT with a message: the shared counter of expect.hpp
#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        if (!(cond)) {                                                               \
            ++failures;                                                              \
            std::printf("FAIL %s:%d %s: ", __func__, __LINE__, #cond);              \
            std::printf(__VA_ARGS__);                                                \
            std::printf("\n");                                                       \
        }                                                                            \
    } while (0)

// ---- shard ranges and cut ---------------------------------------------------------------------------------------------------
void shard_ranges() {
    const int64_t totals[] = {0, 1, 101, 40000000};
    const int shard_counts[] = {1, 2, 3, 8};
    for (int64_t total : totals)
        for (int n : shard_counts) {
            std::vector<int64_t> first(n), count(n);
            int64_t next = 0;
            for (int r = 0; r < n; ++r) {
                CHECK(ukfb::shard_range(total, n, r, &first[r], &count[r]) == UKFB_OK, "total %lld", (long long)total);
                CHECK(first[r] == next, "total %lld n %d shard %d: first %lld, expected %lld", (long long)total, n, r,
                      (long long)first[r], (long long)next);
                // sizes differ by one at most, the larger shards first
                CHECK(count[r] == total / n + (r < total % n ? 1 : 0), "total %lld n %d shard %d: count %lld", (long long)total, n, r,
                      (long long)count[r]);
                next = first[r] + count[r];
            }
            CHECK(next == total, "total %lld n %d: shards cover %lld", (long long)total, n, (long long)next);
            // cut against a brute-force intersection (small totals: every range; the large one: ranges around the shard edges)
            std::vector<int64_t> probes;
            if (total <= 101) {
                for (int64_t a = 0; a <= total; ++a) probes.push_back(a);
            } else {
                for (int r = 0; r < n; ++r)
                    for (int64_t d = -2; d <= 2; ++d) probes.push_back(std::min(total, std::max<int64_t>(0, first[r] + d)));
                probes.push_back(total);
            }
            for (int64_t a : probes)
                for (int64_t b : probes) {
                    if (b < a) continue;
                    for (int r = 0; r < n; ++r) {
                        const ukfb::Cut c = ukfb::cut(first[r], count[r], a, b - a);
                        int64_t lo = -1, len = 0;   // brute force over the [a, b) x shard r overlap
                        const int64_t hi_scan = std::min(b, first[r] + count[r]);
                        if (total <= 101) {
                            for (int64_t f = a; f < b; ++f)
                                if (f >= first[r] && f < first[r] + count[r]) {
                                    if (lo < 0) lo = f;
                                    ++len;
                                }
                        } else if (std::max(a, first[r]) < hi_scan) {
                            lo = std::max(a, first[r]);
                            len = hi_scan - lo;
                        }
                        CHECK(c.len == len, "[%lld, %lld) shard %d: len %lld, expected %lld", (long long)a, (long long)b, r,
                              (long long)c.len, (long long)len);
                        if (len) {
                            CHECK(c.src == lo - a && c.dst == lo - first[r], "[%lld, %lld) shard %d: src %lld dst %lld", (long long)a,
                                  (long long)b, r, (long long)c.src, (long long)c.dst);
                        }
                    }
                }
        }
    CHECK(ukfb::shard_range(-1, 2, 0, nullptr, nullptr) == UKFB_ERR_INVALID_ARG, "negative total");
    CHECK(ukfb::shard_range(10, 0, 0, nullptr, nullptr) == UKFB_ERR_INVALID_ARG, "no shards");
    CHECK(ukfb::shard_range(10, 2, 2, nullptr, nullptr) == UKFB_ERR_INVALID_ARG, "shard past the end");
}

// ---- owner pass ---------------------------------------------------------------------------------------------------------------
void owner_pass_case(int64_t total, int n) {
    std::vector<int64_t> first(n), count(n);
    for (int r = 0; r < n; ++r) ukfb::shard_range(total, n, r, &first[r], &count[r]);
    // every filter once in both directions, the shard edges again, then a scramble
    std::vector<int64_t> filter;
    for (int64_t f = 0; f < total; ++f) filter.push_back(f);
    for (int64_t f = total - 1; f >= 0; --f) filter.push_back(f);
    for (int r = 0; r < n; ++r) {
        filter.push_back(first[r]);
        filter.push_back(first[r] + count[r] - 1);
    }
    for (int64_t k = 0; k < 3 * total; ++k) filter.push_back((k * 7919 + 13) % total);
    std::vector<uint8_t> owner(filter.size());
    std::vector<size_t> counts(size_t(n), 12345);
    CHECK(ukfb::route_events(filter.data(), int64_t(filter.size()), total, first.data(), count.data(), size_t(n), owner.data(),
                             counts.data()) == UKFB_OK, "total %lld n %d", (long long)total, n);
    // every event to the shard that holds its filter, counted once: the routing pass then collects each shard's events in
    // arrival order, a stable partition
    std::vector<size_t> seen(size_t(n), 0);
    for (size_t i = 0; i < filter.size(); ++i) {
        const int r = owner[i];
        CHECK(r < n && filter[i] >= first[r] && filter[i] < first[r] + count[r], "total %lld n %d: filter %lld routed to %d",
              (long long)total, n, (long long)filter[i], r);
        if (r < n) ++seen[size_t(r)];
    }
    size_t sum = 0;
    for (int r = 0; r < n; ++r) {
        CHECK(seen[size_t(r)] == counts[size_t(r)], "total %lld n %d shard %d: counts %zu, owners %zu", (long long)total, n, r,
              counts[size_t(r)], seen[size_t(r)]);
        sum += counts[size_t(r)];
    }
    CHECK(sum == filter.size(), "total %lld n %d: %zu of %zu events routed", (long long)total, n, sum, filter.size());
    for (int64_t bad : {int64_t(-1), total}) {
        std::vector<int64_t> f2 = {0, bad, total - 1};
        std::vector<uint8_t> o2(f2.size());
        CHECK(ukfb::route_events(f2.data(), 3, total, first.data(), count.data(), size_t(n), o2.data(), counts.data()) ==
                  UKFB_ERR_OUT_OF_RANGE, "total %lld n %d: index %lld accepted", (long long)total, n, (long long)bad);
    }
}

void owner_pass() {
    owner_pass_case(101, 2);
    owner_pass_case(101, 3);
    owner_pass_case(101, 8);
    owner_pass_case(7, 7);
    owner_pass_case(255, 255);
    owner_pass_case(1000, 255);
    owner_pass_case(2 * 255 + 254, 255);
}

// ---- configuration ------------------------------------------------------------------------------------------------------------
ukfb_config defaults() {
    ukfb_config c{};
    c.mean_tol = 1e-6;
    c.mean_max_iter = 10000;
    c.gate_chi2 = -1.0;
    c.min_time_delta = 1.0e-9;
    c.max_time_delta = std::numeric_limits<double>::max();
    c.lanes_per_filter = 16;
    c.bucket_models = 1;
    c.split_streams = 1;
    return c;
}

void expect_config(int prec, bool generic, ukfb_config c, int rc, const char* msg, int lanes_after, int line) {
    const ukfb::Verdict v = ukfb::check_config(prec, generic, c);
    CHECK(v.rc == rc, "line %d: rc %d, expected %d", line, v.rc, rc);
    if (msg) CHECK(v.msg && std::strcmp(v.msg, msg) == 0, "line %d: text '%s'", line, v.msg ? v.msg : "(null)");
    if (!msg) CHECK(v.msg == nullptr, "line %d: text '%s' on success", line, v.msg);
    if (rc == UKFB_OK) CHECK(c.lanes_per_filter == lanes_after, "line %d: lanes_per_filter %d", line, c.lanes_per_filter);
}

void config() {
    const char* const LANES = "lanes_per_filter must be 16, 32 or 64";
    const char* const F64 = "lanes_per_filter 32 / 64 in fp64 is a diagnostic build option (make GENERIC_F64=1)";
    const char* const WIDE_LAYOUT = "wide_arithmetic runs on the tuned layout only (lanes_per_filter 16)";
    for (int prec : {int(UKFB_F64), int(UKFB_F32)})
        for (bool generic : {false, true}) {
            ukfb_config c = defaults();
            expect_config(prec, generic, c, UKFB_OK, nullptr, 16, __LINE__);
            c.lanes_per_filter = 0;
            expect_config(prec, generic, c, UKFB_OK, nullptr, 16, __LINE__);
            for (int bad : {-16, 1, 8, 15, 17, 48, 128}) {
                c = defaults();
                c.lanes_per_filter = bad;
                expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, LANES, 0, __LINE__);
            }
            for (int lanes : {32, 64}) {
                c = defaults();
                c.lanes_per_filter = lanes;
                const bool built = prec == UKFB_F32 || generic;
                expect_config(prec, generic, c, built ? UKFB_OK : UKFB_ERR_INVALID_ARG, built ? nullptr : F64, lanes, __LINE__);
                CHECK(ukfb::layout_supported(prec, lanes, generic) == built, "prec %d lanes %d generic %d", prec, lanes, int(generic));
                // wide arithmetic: fp32 engines on the tuned layout only (fp64 engines ignore it)
                c.wide_arithmetic = 1;
                if (prec == UKFB_F32) expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, WIDE_LAYOUT, 0, __LINE__);
                else expect_config(prec, generic, c, built ? UKFB_OK : UKFB_ERR_INVALID_ARG, built ? nullptr : F64, lanes, __LINE__);
            }
            c = defaults();
            c.mean_max_iter = 0;
            expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, "mean_max_iter must be >= 1", 0, __LINE__);
            c = defaults();
            c.wide_arithmetic = 2;
            expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, "wide_arithmetic must be 0 or 1", 0, __LINE__);
            c.wide_arithmetic = 1;
            expect_config(prec, generic, c, UKFB_OK, nullptr, 16, __LINE__);
            c = defaults();
            c.full_update_check = -1;
            expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, "full_update_check must be 0 or 1", 0, __LINE__);
            // the order of the checks: the first failing field names the error
            c = defaults();
            c.lanes_per_filter = 7;
            c.mean_max_iter = 0;
            c.wide_arithmetic = 5;
            expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, LANES, 0, __LINE__);
            c.lanes_per_filter = 16;
            expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, "mean_max_iter must be >= 1", 0, __LINE__);
            c.mean_max_iter = 1;
            c.full_update_check = 3;
            expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG, "wide_arithmetic must be 0 or 1", 0, __LINE__);
            c.wide_arithmetic = 1;
            c.lanes_per_filter = 32;
            expect_config(prec, generic, c, UKFB_ERR_INVALID_ARG,
                          (prec == UKFB_F64 && !generic) ? F64 : "full_update_check must be 0 or 1", 0, __LINE__);
        }
    CHECK(!ukfb::layout_supported(7, 16, true), "unknown precision");
}

// ---- process noise ------------------------------------------------------------------------------------------------------------
std::vector<double> diag(const std::vector<double>& d) {
    const size_t D = d.size();
    std::vector<double> A(D * D, 0.0);
    for (size_t i = 0; i < D; ++i) A[i * D + i] = d[i];
    return A;
}
const double ACC_ID[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

void noise_builtin() {
    for (int model : {int(UKFB_MODEL_POSE), int(UKFB_MODEL_ORIENT)}) {
        const int D = model == UKFB_MODEL_POSE ? 12 : 13;
        const std::vector<double> zero(size_t(D) * D, 0.0);   // the engine's default noise
        CHECK(ukfb::short_update_ok(model, D, zero.data(), ACC_ID), "model %d: zero noise", model);
        CHECK(ukfb::rotated_blocks_isotropic(zero.data(), D), "model %d: zero noise is isotropic", model);
        std::vector<double> d(size_t(D), 1e-5);
        for (int i = 0; i < 3; ++i) {
            d[size_t(i)] = 0.01;
            d[size_t(3 + i)] = 0.001;
        }
        std::vector<double> R = diag(d);
        CHECK(ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: isotropic diagonal", model);
        CHECK(ukfb::rotated_blocks_isotropic(R.data(), D), "model %d: isotropic diagonal", model);
        R[1 * D + 1] = 0.02;   // anisotropic rotated block: still PSD and uncoupled
        CHECK(!ukfb::rotated_blocks_isotropic(R.data(), D), "model %d: anisotropic block", model);
        CHECK(ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: anisotropic diagonal", model);
        R[1 * D + 1] = 0.01;
        R[0 * D + 1] = R[1 * D + 0] = 1e-4;   // coupling inside a rotated block: allowed, not isotropic
        CHECK(!ukfb::rotated_blocks_isotropic(R.data(), D), "model %d: off-diagonal in a block", model);
        CHECK(ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: in-block coupling", model);
        R[0 * D + 1] = R[1 * D + 0] = 0.0;
        R[0 * D + 3] = R[3 * D + 0] = 1e-4;   // coupling between the two rotated blocks: PSD, but not after rotation
        CHECK(!ukfb::rotated_blocks_uncoupled(R.data(), D), "model %d: block coupling", model);
        CHECK(!ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: block coupling accepted", model);
        R[0 * D + 3] = R[3 * D + 0] = 0.0;
        R[D * D - 1] = -1e-3;   // not PSD
        CHECK(!ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: negative pivot accepted", model);
        R[D * D - 1] = 1e-5;
        R[2 * D + 2] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: NaN on the diagonal accepted", model);
        R[2 * D + 2] = 0.01;
        R[(D - 1) * D + (D - 2)] = std::numeric_limits<double>::quiet_NaN();   // lower triangle, outside the rotated blocks
        CHECK(!ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: NaN below the diagonal accepted", model);
        R[(D - 1) * D + (D - 2)] = 0.0;
        CHECK(ukfb::short_update_ok(model, D, R.data(), ACC_ID), "model %d: restored", model);
        // a PSD R whose acceleration-branch form (velocity block = 2 acc_cov) is indefinite: rejected for Pose only
        const double acc_indef[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
        CHECK(ukfb::short_update_ok(model, D, R.data(), acc_indef) == (model != UKFB_MODEL_POSE), "model %d: indefinite acc_cov",
              model);
        // acceleration branch with cross terms into the velocity block: R itself PSD, Ra indefinite
        std::vector<double> Rc = R;
        for (int k = 6; k < 9; ++k) Rc[size_t(k) * D + k] = 1.0;
        Rc[9 * D + 6] = Rc[6 * D + 9] = 3e-3;   // |c| <= sqrt(1 * 1e-5): PSD with the raw velocity block
        const double acc_small[9] = {1e-9, 0, 0, 0, 1e-9, 0, 0, 0, 1e-9};
        CHECK(ukfb::is_psd(Rc.data(), D), "model %d: raw R with velocity coupling is PSD", model);
        CHECK(ukfb::short_update_ok(model, D, Rc.data(), acc_small) == (model != UKFB_MODEL_POSE),
              "model %d: acc branch with coupling", model);
    }
}

// cases from synth.py (tests/test_host_logic.py writes them)
void noise_file(const char* path) {
    std::ifstream in(path);
    CHECK(in.good(), "cannot read %s", path);
    int cases = 0;
    std::string name;
    int model = 0, D = 0, expected = 0;
    while (in >> name >> model >> D >> expected) {
        std::vector<double> R(size_t(D) * D);
        for (double& v : R) in >> v;
        CHECK(!in.fail(), "%s: short record", name.c_str());
        CHECK(ukfb::short_update_ok(model, D, R.data(), ACC_ID) == (expected != 0), "%s: short update %s", name.c_str(),
              expected ? "refused" : "allowed");
        ++cases;
    }
    CHECK(cases >= 4, "%s: %d cases", path, cases);
}

// ---- multi-cycle plans --------------------------------------------------------------------------------------------------------
void plans() {
    CHECK(ukfb::check_cycle_args(0, 1, 0).rc == UKFB_OK, "cycles 0");
    const int bad[4][3] = {{-1, 1, 0}, {1, 0, 0}, {1, 2, -1}, {1, 2, 2}};   // cycles, slots, first_slot
    for (const auto& a : bad) {
        const ukfb::Verdict v = ukfb::check_cycle_args(a[0], a[1], a[2]);
        CHECK(v.rc == UKFB_ERR_INVALID_ARG && v.msg && std::strcmp(v.msg, "cycles >= 0, slots >= 1, 0 <= first_slot < slots") == 0,
              "cycles %d slots %d first_slot %d", a[0], a[1], a[2]);
    }
    for (int cycles : {0, 1, 31, 32, 33, 65})
        for (int slots : {1, 3, 32, 70})
            for (int first_slot : {0, slots - 1, slots / 2})
                for (bool tuned : {true, false})
                    for (bool schedule : {true, false}) {
                        const ukfb::CyclePlan p(cycles, slots, first_slot, tuned, schedule);
                        CHECK(p.multi == tuned, "multi");
                        int next = 0;
                        for (int k = 0; k < p.launches(); ++k) {
                            const ukfb::CycleLaunch l = p[k];
                            CHECK(l.first_cycle == next && l.cycles >= 1, "cycles %d launch %d: first %d count %d", cycles, k,
                                  l.first_cycle, l.cycles);
                            CHECK(l.slot == (first_slot + l.first_cycle) % slots, "cycles %d launch %d: slot %d", cycles, k, l.slot);
                            CHECK(l.status_accumulate == (k > 0), "cycles %d launch %d: status_accumulate", cycles, k);
                            // the kernel's schedule arrays hold 32 cycles (ukf_kernel.hpp); the other layouts run one per launch
                            if (!tuned) CHECK(l.cycles == 1, "per-cycle layout: %d cycles in one launch", l.cycles);
                            if (tuned && schedule) CHECK(l.cycles <= 32, "scheduled launch of %d cycles", l.cycles);
                            if (tuned && schedule && k + 1 < p.launches()) CHECK(l.cycles == 32, "short scheduled launch");
                            if (tuned && !schedule) CHECK(p.launches() == 1, "unscheduled multi-cycle call in %d launches", p.launches());
                            next += l.cycles;
                        }
                        CHECK(next == cycles, "cycles %d slots %d tuned %d schedule %d: plan covers %d", cycles, slots, int(tuned),
                              int(schedule), next);
                    }
    // ring slots past INT_MAX cycles must not overflow
    const ukfb::CyclePlan big(std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), std::numeric_limits<int>::max() - 1,
                              false, true);
    const ukfb::CycleLaunch last = big[big.launches() - 1];
    CHECK(last.slot == int((int64_t(big.first_slot) + last.first_cycle) % big.slots), "slot of the last launch");
}

// ---- sizing -------------------------------------------------------------------------------------------------------------------
void sizing() {
    for (int64_t n : {int64_t(1), int64_t(16384), int64_t(2097152), int64_t(2097153), int64_t(40000000), int64_t(0x7fffffff - 16)}) {
        const ukfb::BucketGeometry g = ukfb::bucket_geometry(n);
        CHECK(int64_t(g.blocks) * ukfb::BK_BLOCK >= n && int64_t(g.blocks - 1) * ukfb::BK_BLOCK < n, "n %lld: blocks %d", (long long)n,
              g.blocks);
        CHECK(g.list == size_t(n) + 16 && int64_t(g.list) >= g.items, "n %lld: list %zu items %lld", (long long)n, g.list,
              (long long)g.items);
        CHECK(g.count_words == size_t(6) * size_t(g.blocks) + 4, "n %lld: count words", (long long)n);
        CHECK(g.items % 4 == 0 && g.items <= int64_t(0xffffffffu), "n %lld: items %lld", (long long)n, (long long)g.items);
        CHECK(g.inline_scan == (n <= 2048 * int64_t(1024)), "n %lld: inline scan %d", (long long)n, int(g.inline_scan));
        // every split of n into the three classes, each padded to whole wavefronts, fits in items
        for (int64_t a = 0; a < 4; ++a)
            for (int64_t b = 0; b < 4; ++b) {
                if (a + b > n) continue;
                const int64_t c = n - a - b, pad = (a + 3) / 4 * 4 + (b + 3) / 4 * 4 + (c + 3) / 4 * 4;
                CHECK(g.items >= pad, "n %lld classes %lld/%lld/%lld: items %lld < %lld", (long long)n, (long long)a, (long long)b,
                      (long long)c, (long long)g.items, (long long)pad);
            }
    }
    ukfb_config cfg = defaults();
    CHECK(!ukfb::buckets_apply(true, cfg, 16383) && ukfb::buckets_apply(true, cfg, 16384), "bucket threshold");
    CHECK(ukfb::buckets_apply(true, cfg, 0x7fffffff - 16) && !ukfb::buckets_apply(true, cfg, 0x7fffffff - 15), "bucket cap");
    CHECK(!ukfb::buckets_apply(false, cfg, 1 << 20), "uniform model");
    cfg.lanes_per_filter = 32;
    CHECK(!ukfb::buckets_apply(true, cfg, 1 << 20), "one-wavefront layout");
    cfg = defaults();
    cfg.bucket_models = 0;
    CHECK(!ukfb::buckets_apply(true, cfg, 1 << 20), "bucket_models off");

    // the events workspace covers the carved layout (sort temporaries excepted) for every size of a call
    for (int64_t n : {int64_t(1), int64_t(2), int64_t(255), int64_t(1) << 20, int64_t(40000000), int64_t(0x7fffffff)}) {
        for (size_t tsize : {size_t(4), size_t(8)}) {
            ukfb::Carver c(nullptr);
            const size_t ne = size_t(n);
            for (int k = 0; k < 4; ++k) c.take<uint32_t>(ne);   // idx a..d
            c.take<int64_t>(ne); c.take<int64_t>(ne); c.take<uint32_t>(ne); c.take<uint32_t>(ne);   // time and filter keys
            for (int k = 0; k < 4; ++k) c.take<uint32_t>(ne);   // head, start, rank, rank_sorted
            c.take<uint32_t>(ne + 1); c.take<int32_t>(ne); c.take<int64_t>(ne); c.take<int32_t>(ne);   // off, compact events
            c.take<char>(3 * ne * tsize); c.take<char>(9 * ne * tsize); c.take<uint32_t>(2);
            CHECK(ukfb::events_workspace_bytes(n) >= c.used, "n %lld tsize %zu: workspace %zu < layout %zu", (long long)n, tsize,
                  ukfb::events_workspace_bytes(n), c.used);
            CHECK(c.take<char>(1) == nullptr, "a measuring carver hands out no memory");
        }
    }
    char buf[1024];
    ukfb::Carver c(buf);
    CHECK(c.take<int64_t>(3) == reinterpret_cast<int64_t*>(buf) && c.take<char>(1) == buf + 256 && c.used == 512, "carver offsets");

    CHECK(ukfb::split_first_half(16384) == 8192 && ukfb::split_first_half(16385) == 8192 && ukfb::split_first_half(16386) == 8196 && ukfb::split_first_half(16390) == 8196,
          "first half");
    for (int64_t n : {int64_t(16384), int64_t(16387), int64_t(100001), int64_t(262143)}) {
        const int64_t h = ukfb::split_first_half(n);
        CHECK(h % 4 == 0 && h >= n / 2 && h < n, "n %lld: first half %lld", (long long)n, (long long)h);
    }
    CHECK(ukfb::split_launch(false, false, true, true, 16384, 262144), "split at the lower bound");
    CHECK(!ukfb::split_launch(false, false, true, true, 16383, 262144), "below");
    CHECK(!ukfb::split_launch(false, false, true, true, 262144, 262144), "at the upper bound");
    CHECK(!ukfb::split_launch(true, false, true, true, 65536, 262144), "indirect");
    CHECK(!ukfb::split_launch(false, true, true, true, 65536, 262144), "no_split");
    CHECK(!ukfb::split_launch(false, false, false, true, 65536, 262144), "no second stream");
    CHECK(!ukfb::split_launch(false, false, true, false, 65536, 262144), "split_streams off");
}

// ---- measurement models -------------------------------------------------------------------------------------------------------
void models() {
    for (int m = -3; m <= 12; ++m) {
        CHECK(ukfb::meas_model_ok(UKFB_MODEL_POSE, m) == (m >= 0 && m <= 8), "pose %d", m);
        CHECK(ukfb::meas_model_ok(UKFB_MODEL_ORIENT, m) == (m == 9), "orient %d", m);
        CHECK(ukfb::update_class(UKFB_MODEL_POSE, m) == ((m < 0 || m > 8) ? 0 : (m == 3 ? 2 : 1)), "pose class %d", m);
        CHECK(ukfb::update_class(UKFB_MODEL_ORIENT, m) == (m == 9 ? 2 : 0), "orient class %d", m);
    }
}

// ---- packed covariances -------------------------------------------------------------------------------------------------------
// D = 12, 13: the two models; 15: the largest the 16-lane kernels admit (S = D + 1 <= 16).  The strict upper triangle of every input is NaN:
// pack_lower must not read it.  count = 0 works on zero-length vectors, so that ASan sees any access.
void packing() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int D : {12, 13, 15})
        for (size_t count : {size_t(0), size_t(3)}) {
            const size_t d = size_t(D), PK = d * (d + 1) / 2;
            std::vector<double> A(count * d * d), packed(count * PK, nan), back(count * d * d, nan);
            for (size_t i = 0; i < count; ++i)
                for (size_t r = 0; r < d; ++r)
                    for (size_t c = 0; c < d; ++c) A[(i * d + r) * d + c] = c <= r ? 1.0 / double(1 + i * d * d + r * d + c) : nan;
            ukfb::pack_lower(A.data(), count, D, packed.data());
            size_t k = 0;   // the packed order: matrix by matrix, row by row, columns 0 ... r
            for (size_t i = 0; i < count; ++i)
                for (size_t r = 0; r < d; ++r)
                    for (size_t c = 0; c <= r; ++c, ++k)
                        CHECK(std::isfinite(packed[k]) && std::memcmp(&packed[k], &A[(i * d + r) * d + c], sizeof(double)) == 0,
                              "D %d matrix %zu (%zu, %zu): packed %g", D, i, r, c, packed[k]);
            CHECK(k == packed.size(), "D %d count %zu: %zu packed entries of %zu", D, count, k, packed.size());
            ukfb::unpack_symmetric(packed.data(), count, D, back.data());
            for (size_t i = 0; i < count; ++i)
                for (size_t r = 0; r < d; ++r)
                    for (size_t c = 0; c < d; ++c) {
                        const double& lower = A[(i * d + std::max(r, c)) * d + std::min(r, c)];   // A's lower triangle mirrored
                        CHECK(std::memcmp(&back[(i * d + r) * d + c], &lower, sizeof(double)) == 0, "D %d matrix %zu (%zu, %zu): unpacked %g",
                              D, i, r, c, back[(i * d + r) * d + c]);
                        CHECK(std::memcmp(&back[(i * d + r) * d + c], &back[(i * d + c) * d + r], sizeof(double)) == 0,
                              "D %d matrix %zu (%zu, %zu): not symmetric", D, i, r, c);
                    }
        }
}

// ---- kernel level -------------------------------------------------------------------------------------------------------------
// The table as launch_row16 (ukf_launch.inc.hpp) wrote it before the logic moved to ukf_host.hpp, restated literally.
int level_before(int model, const ukfb::LaunchFacts& f) {
    const bool streams_only = !f.timestamps && !f.dt_array && !f.active && !f.status_accumulate && !f.gate &&
                              (!f.multi || !f.schedule) && (!f.indirect || f.bucketed);
    const bool full3 = !f.meas_per_filter && (model != 0 ? f.meas_uniform == 9
                                                         : (f.meas_uniform == 0 || f.meas_uniform == 4 || f.meas_uniform == 8));
    int level = 0;
    if (streams_only) {
        if (f.indirect) level = 1;
        else if (f.multi) level = full3 ? 2 : 0;
        else if (!f.update) level = 2;
        else level = full3 ? 2 : 1;
    }
    return level;
}

void kernel_levels() {
    int rows = 0;
    for (int model : {int(UKFB_MODEL_POSE), int(UKFB_MODEL_ORIENT)})
        for (int meas = -1; meas <= 10; ++meas)
            for (unsigned bits = 0; bits < (1u << 11); ++bits) {
                ukfb::LaunchFacts f;
                f.timestamps = bits & 1; f.dt_array = bits & 2; f.active = bits & 4; f.status_accumulate = bits & 8; f.gate = bits & 16;
                f.indirect = bits & 32; f.bucketed = bits & 64; f.multi = bits & 128; f.schedule = bits & 256; f.update = bits & 512;
                f.meas_per_filter = bits & 1024; f.meas_uniform = meas;
                const int got = ukfb::kernel_level(model, f), want = level_before(model, f);
                CHECK(got == want, "model %d meas %d facts 0x%03x: level %d, table %d", model, meas, bits, got, want);
                ++rows;
            }
    CHECK(rows == 2 * 12 * 2048, "rows %d", rows);
    // named rows: the launches the GPU tests assert by kernel name
    ukfb::LaunchFacts f;
    f.update = true;
    f.meas_uniform = UKFB_MEAS_POS3;
    CHECK(ukfb::kernel_level(UKFB_MODEL_POSE, f) == 2, "plain Pose position cycle");
    f.meas_uniform = UKFB_MEAS_ORIENT_SO3;
    CHECK(ukfb::kernel_level(UKFB_MODEL_POSE, f) == 1, "streams-only Pose orientation cycle");
    f.meas_uniform = UKFB_MEAS_ORIENT_BODYVEL3;
    CHECK(ukfb::kernel_level(UKFB_MODEL_ORIENT, f) == 2, "plain Orient cycle");
    f.timestamps = true;
    CHECK(ukfb::kernel_level(UKFB_MODEL_ORIENT, f) == 0, "per-filter timestamps keep the general kernel");
    f.timestamps = false;
    f.indirect = true;
    f.meas_per_filter = true;
    CHECK(ukfb::kernel_level(UKFB_MODEL_ORIENT, f) == 0, "event rounds keep the general kernel");
    f.bucketed = true;
    CHECK(ukfb::kernel_level(UKFB_MODEL_ORIENT, f) == 1, "bucketed list: streams only");
    ukfb::LaunchFacts m;
    m.multi = true;
    m.update = true;
    m.meas_uniform = UKFB_MEAS_VEL3;
    CHECK(ukfb::kernel_level(UKFB_MODEL_POSE, m) == 2, "plain multi-cycle");
    m.schedule = true;
    CHECK(ukfb::kernel_level(UKFB_MODEL_POSE, m) == 0, "scheduled multi-cycle");
    ukfb::LaunchFacts p;   // prediction only
    CHECK(ukfb::kernel_level(UKFB_MODEL_POSE, p) == 2, "prediction only");
    p.gate = true;
    CHECK(ukfb::kernel_level(UKFB_MODEL_POSE, p) == 0, "gate on");
}

// ---- bounded waits: the polling loop against scripted queries, and the UKFB_WAIT_TIMEOUT_S parser -----------------------------
void waits() {
    enum Answer { READY = 0, NOT_READY = 7, BROKEN = 3 };
    int queries = 0;
    // ready_at: the number of the first query (from 1) that no longer answers NOT_READY; 0: never
    auto scripted = [&queries](int ready_at, Answer then) {
        queries = 0;
        return [&queries, ready_at, then] { return ++queries >= ready_at && ready_at > 0 ? then : NOT_READY; };
    };
    {
        const ukfb::Waited<Answer> w = ukfb::wait_polling(scripted(1, READY), NOT_READY, 100, 5.0);
        CHECK(!w.gave_up && w.result == READY && queries == 1, "ready at the first poll: gave_up %d result %d queries %d", w.gave_up,
              w.result, queries);
    }
    for (int k : {1, 7, 99}) {   // ready after k polls inside the spin: exactly k + 1 queries
        const ukfb::Waited<Answer> w = ukfb::wait_polling(scripted(k + 1, READY), NOT_READY, 100, 5.0);
        CHECK(!w.gave_up && w.result == READY && queries == k + 1, "k %d: gave_up %d result %d queries %d", k, w.gave_up, w.result,
              queries);
    }
    {   // ready only after the spin phase has ended (10 spins, then the sleeping polls)
        const ukfb::Waited<Answer> w = ukfb::wait_polling(scripted(25, READY), NOT_READY, 10, 5.0);
        CHECK(!w.gave_up && w.result == READY && queries == 25, "past the spin: gave_up %d result %d queries %d", w.gave_up, w.result,
              queries);
    }
    {   // an error is returned at once, in the spin and past it
        const ukfb::Waited<Answer> w = ukfb::wait_polling(scripted(1, BROKEN), NOT_READY, 100, 5.0);
        CHECK(!w.gave_up && w.result == BROKEN && queries == 1, "error: gave_up %d result %d queries %d", w.gave_up, w.result, queries);
        const ukfb::Waited<Answer> v = ukfb::wait_polling(scripted(12, BROKEN), NOT_READY, 10, 5.0);
        CHECK(!v.gave_up && v.result == BROKEN && queries == 12, "late error: gave_up %d result %d queries %d", v.gave_up, v.result,
              queries);
    }
    {   // never ready: gives up, no sooner than the timeout and no later than the timeout plus 1 s
        const double timeout = 0.05;
        const auto t0 = std::chrono::steady_clock::now();
        const ukfb::Waited<Answer> w = ukfb::wait_polling(scripted(0, READY), NOT_READY, 100, timeout);
        const double took = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        CHECK(w.gave_up && w.result == NOT_READY, "never ready: gave_up %d result %d", w.gave_up, w.result);
        CHECK(took >= timeout && took <= timeout + 1.0, "never ready: took %.4f s", took);
        CHECK(queries > 100, "never ready: %d queries", queries);
    }
    CHECK(ukfb::wait_timeout_seconds(nullptr) == 120.0, "unset");
    CHECK(ukfb::wait_timeout_seconds("0") == 120.0, "0");
    CHECK(ukfb::wait_timeout_seconds("-3") == 120.0, "-3");
    CHECK(ukfb::wait_timeout_seconds("abc") == 120.0, "abc");
    CHECK(ukfb::wait_timeout_seconds("7.5") == 7.5, "7.5");
}
}  // namespace

int main(int argc, char** argv) {
    shard_ranges();
    owner_pass();
    config();
    noise_builtin();
    if (argc > 1) noise_file(argv[1]);
    else CHECK(false, "no noise case file given");
    plans();
    sizing();
    models();
    packing();
    kernel_levels();
    waits();
    return finish();
}
