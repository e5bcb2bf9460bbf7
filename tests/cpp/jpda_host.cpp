// jpda_host.cpp -- the host decisions of the joint association (ukf_host.hpp) on the CPU (g++ under ASan / UBSan, compiled by
// tests/test_jpda_host.py): one case per argument error of include/ukf_batch_jpda.h and their order, the segment rule with the
// limit of six tracks, the rules of a pair, the dimension a model id counts as, the checks of the update with given weights,
// and the launch geometry.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

int main() {
    using namespace ukfb;
    char buf = 0;
    int32_t i32 = 0;
    uint32_t u32 = 0;
    double f64 = 0.0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int64_t CAP = 1022;
    const ukfb_pda_rule rule{0.9, 0.9999, 0.9989, 2.0, 300.0};
    ukfb_jpda_in in{};
    in.loglik_dev = &buf; in.candidates = 5; in.scenes = 10; in.tracks_per_scene = 4; in.gate = -1.0; in.model_uniform = 4;
    ukfb_jpda_out out{};
    out.beta = &buf;
    EXPECT(check_jpda_args(CAP, &in, &rule, &out).rc == UKFB_OK);
    {   // every output alone is something to compute; none is not
        ukfb_jpda_out o{};
        EXPECT(check_jpda_args(CAP, &in, &rule, &o).rc == UKFB_ERR_INVALID_ARG);
        EXPECT(check_jpda_args(CAP, &in, &rule, nullptr).rc == UKFB_ERR_INVALID_ARG);
        o = {}; o.beta0 = &buf; EXPECT(check_jpda_args(CAP, &in, &rule, &o).rc == UKFB_OK);
        o = {}; o.free = &f64; EXPECT(check_jpda_args(CAP, &in, &rule, &o).rc == UKFB_OK);
        o = {}; o.log_z = &f64; EXPECT(check_jpda_args(CAP, &in, &rule, &o).rc == UKFB_OK);
        o = {}; o.scene_status = &u32; EXPECT(check_jpda_args(CAP, &in, &rule, &o).rc == UKFB_OK);
    }
    {   // the rule first, whatever else is wrong: NULL, out of range, P_D P_G >= 1
        ukfb_jpda_in a = in;
        a.candidates = 99;
        Verdict v = check_jpda_args(CAP, &a, nullptr, &out);
        EXPECT(v.rc == UKFB_ERR_INVALID_ARG && v.msg != nullptr);
        EXPECT(check_jpda_args(CAP, nullptr, nullptr, nullptr).rc == UKFB_ERR_INVALID_ARG);
        ukfb_pda_rule r = rule;
        r.p_detect = 0.0; EXPECT(check_jpda_args(CAP, &a, &r, &out).rc == UKFB_ERR_INVALID_ARG);
        r = rule; r.p_detect = 1.5; EXPECT(check_jpda_args(CAP, &in, &r, &out).rc == UKFB_ERR_INVALID_ARG);
        r = rule; r.p_gate_m3 = nan; EXPECT(check_jpda_args(CAP, &in, &r, &out).rc == UKFB_ERR_INVALID_ARG);
        r = rule; r.clutter_m1 = 0.0; EXPECT(check_jpda_args(CAP, &in, &r, &out).rc == UKFB_ERR_INVALID_ARG);
        r = rule; r.clutter_m3 = inf; EXPECT(check_jpda_args(CAP, &in, &r, &out).rc == UKFB_ERR_INVALID_ARG);
        r = rule; r.p_detect = 1.0; r.p_gate_m1 = 1.0; EXPECT(check_jpda_args(CAP, &in, &r, &out).rc == UKFB_ERR_INVALID_ARG);
        r = rule; r.p_detect = 1.0; r.p_gate_m3 = 1.0; EXPECT(check_jpda_args(CAP, &in, &r, &out).rc == UKFB_ERR_INVALID_ARG);
    }
    {   // INVALID_ARG, each with a message
        Verdict v = check_jpda_args(CAP, nullptr, &rule, &out);
        EXPECT(v.rc == UKFB_ERR_INVALID_ARG && v.msg != nullptr);
        ukfb_jpda_in a = in;
        a.loglik_dev = nullptr; v = check_jpda_args(CAP, &a, &rule, &out); EXPECT(v.rc == UKFB_ERR_INVALID_ARG && v.msg != nullptr);
        // a gate needs maha; no gate (< 0 or NaN) does not
        for (double g : {0.0, 16.0, inf}) {
            a = in; a.gate = g; v = check_jpda_args(CAP, &a, &rule, &out); EXPECT(v.rc == UKFB_ERR_INVALID_ARG && v.msg != nullptr);
            a.maha_dev = &buf; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        }
        for (double g : {-1.0, nan, -inf}) {
            a = in; a.gate = g; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        }
        a = in; a.model_uniform = -1; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);   // an id of no engine: m = 3
    }
    {   // OUT_OF_RANGE, behind the INVALID_ARG clauses
        ukfb_jpda_in a = in;
        for (int bad : {0, -1, 33, 1 << 30}) {
            a = in; a.candidates = bad;
            const Verdict v = check_jpda_args(CAP, &a, &rule, &out);
            EXPECT(v.rc == UKFB_ERR_OUT_OF_RANGE && v.msg != nullptr);
            a.loglik_dev = nullptr; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_ERR_INVALID_ARG);
        }
        a = in; a.candidates = 1; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        a = in; a.candidates = 32; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        for (int bad : {0, -1, 7, 32}) {
            a = in; a.tracks_per_scene = bad; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_ERR_OUT_OF_RANGE);
            a.scene_start_dev = &i32; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);     // ragged mode: not read
        }
        a = in; a.tracks_per_scene = 6; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        a = in; a.scenes = -1; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_ERR_OUT_OF_RANGE);
        a = in; a.scenes = 0; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        a = in; a.tracks_per_scene = 4; a.scenes = 256; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        a.scenes = 257; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_ERR_OUT_OF_RANGE);
        a = in; a.tracks_per_scene = 6; a.scenes = 171; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        a.scenes = 172; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_ERR_OUT_OF_RANGE);
        a = in; a.scene_start_dev = &i32; a.scenes = 1023; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_OK);
        a.scenes = 1024; EXPECT(check_jpda_args(CAP, &a, &rule, &out).rc == UKFB_ERR_OUT_OF_RANGE);
    }
    // the segment rule: the assignment's decides BAD_SCENE, then the limit of six
    EXPECT(jpda_segment_status(0, 0, CAP) == UKFB_JPDA_OK && jpda_segment_status(0, 6, CAP) == UKFB_JPDA_OK);
    EXPECT(jpda_segment_status(1016, 1022, CAP) == UKFB_JPDA_OK && jpda_segment_status(1022, 1022, CAP) == UKFB_JPDA_OK);
    EXPECT(jpda_segment_status(0, 7, CAP) == UKFB_JPDA_TOO_LARGE && jpda_segment_status(10, 19, CAP) == UKFB_JPDA_TOO_LARGE);
    EXPECT(jpda_segment_status(990, 1022, CAP) == UKFB_JPDA_TOO_LARGE);
    EXPECT(jpda_segment_status(-1, 3, CAP) == UKFB_JPDA_BAD_SCENE && jpda_segment_status(1020, 1023, CAP) == UKFB_JPDA_BAD_SCENE);
    EXPECT(jpda_segment_status(5, 4, CAP) == UKFB_JPDA_BAD_SCENE && jpda_segment_status(0, 33, CAP) == UKFB_JPDA_BAD_SCENE);
    EXPECT(jpda_segment_status(-2147483647 - 1, 2147483647, CAP) == UKFB_JPDA_BAD_SCENE);
    EXPECT(jpda_segment_status(2147483647, -2147483647 - 1, CAP) == UKFB_JPDA_BAD_SCENE);
    {   // uniform mode's segments pass the rule for every T0 the check admits
        int64_t a = 0, b = 0;
        for (int t0 = 1; t0 <= UKFB_JPDA_MAX_TRACKS; ++t0) {
            ukfb_jpda_in u = in;
            u.tracks_per_scene = t0;
            const int64_t most = jpda_max_scenes(&u, CAP);
            int64_t covered = 0;
            for (int64_t s = 0; s < most; ++s) {
                assign_uniform_segment(s, t0, CAP, &a, &b);
                EXPECT(jpda_segment_status(a, b, CAP) == UKFB_JPDA_OK && a == covered && b > a);
                covered = b;
            }
            EXPECT(covered == CAP);
        }
    }
    {   // the host-array form's offsets: bad ones are refused, a too-large scene is not (its status says so)
        const std::vector<int32_t> good{0, 0, 5, 14, 14, 1022 - 32, 1022};
        EXPECT(check_assign_offsets(CAP, 3, good.data()).rc == UKFB_OK);
        EXPECT(check_assign_offsets(CAP, 5, good.data()).rc == UKFB_ERR_OUT_OF_RANGE);   // 14 ... 990
        const std::vector<int32_t> back{0, 8, 4, 12};
        EXPECT(check_assign_offsets(CAP, 3, back.data()).rc == UKFB_ERR_OUT_OF_RANGE);
    }
    // a pair
    EXPECT(jpda_finite(0.0) && jpda_finite(-1e300) && !jpda_finite(nan) && !jpda_finite(inf) && !jpda_finite(-inf));
    EXPECT(jpda_gate_on(0.0) && jpda_gate_on(16.0) && !jpda_gate_on(-1.0) && !jpda_gate_on(nan));
    EXPECT(jpda_pair_allowed(-3.0, nan, -1.0) && jpda_pair_allowed(-3.0, 9.0, nan) && jpda_pair_allowed(-3.0, 16.0, 16.0));
    EXPECT(!jpda_pair_allowed(-3.0, 16.0000001, 16.0) && !jpda_pair_allowed(-3.0, nan, 16.0) && !jpda_pair_allowed(-3.0, inf, 16.0));
    EXPECT(!jpda_pair_allowed(nan, 1.0, -1.0) && !jpda_pair_allowed(inf, 1.0, 16.0) && !jpda_pair_allowed(-inf, 1.0, -1.0));
    // m as the PDA kernel takes it
    EXPECT(jpda_kernel_dim(UKFB_MODEL_POSE, UKFB_SENSOR_POSE_RANGE) == 1 && jpda_kernel_dim(UKFB_MODEL_POSE, UKFB_SENSOR_POSE_POINT) == 3);
    EXPECT(jpda_kernel_dim(UKFB_MODEL_POSE, -1) == 3 && jpda_kernel_dim(UKFB_MODEL_POSE, UKFB_SENSOR_ORIENT_VELOCITY) == 3);
    EXPECT(jpda_kernel_dim(UKFB_MODEL_ORIENT, UKFB_SENSOR_POSE_RANGE) == 3 && jpda_kernel_dim(UKFB_MODEL_ORIENT, 99) == 3);
    // the launch: four scenes of one wavefront each per workgroup, no LDS
    EXPECT(jpda_geometry(1).grid == 1 && jpda_geometry(4).grid == 1 && jpda_geometry(5).grid == 2 && jpda_geometry(174763).grid == 43691);
    EXPECT(jpda_geometry(7).lds_bytes == 0 && JPDA_THREADS == 256 && JPDA_SCENES_PER_GROUP == 4 && (1 << UKFB_JPDA_MAX_TRACKS) == 64);
    EXPECT(UKFB_JPDA_LOG_RATIO_MAX == 100.0 && std::exp(6 * UKFB_JPDA_LOG_RATIO_MAX) * std::pow(33.0, 6) < std::numeric_limits<double>::max());

    // ---- the update with given weights
    {
        ukfb_associate_in w{};
        w.candidates = 4; w.z_dev = &buf; w.Q_dev = &buf;
        ukfb_weighted_out wo{};
        wo.status = &u32;
        EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, &w, &buf, 1, &wo).rc == UKFB_OK);
        EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, &w, &buf, 1, nullptr).rc == UKFB_OK);      // commit alone
        EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, &w, &buf, 0, nullptr).rc == UKFB_ERR_INVALID_ARG);
        EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, nullptr, &buf, 1, &wo).rc == UKFB_ERR_INVALID_ARG);
        EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, &w, nullptr, 1, &wo).rc == UKFB_ERR_INVALID_ARG);
        EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_ORIENT_VELOCITY, &w, &buf, 1, &wo).rc == UKFB_ERR_WRONG_MODEL);
        EXPECT(check_weighted_args(UKFB_MODEL_POSE, true, UKFB_SENSOR_ORIENT_VELOCITY, &w, &buf, 1, &wo).rc == UKFB_OK);   // ids per filter
        ukfb_associate_in x = w;
        x.point_per_candidate = 1; EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, &x, &buf, 1, &wo).rc == UKFB_ERR_INVALID_ARG);
        for (int bad : {0, 33, -1}) {
            x = w; x.candidates = bad;
            EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, &x, &buf, 1, &wo).rc == UKFB_ERR_OUT_OF_RANGE);
        }
        x = w; x.z_dev = nullptr; EXPECT(check_weighted_args(UKFB_MODEL_POSE, false, UKFB_SENSOR_POSE_POINT, &x, &buf, 1, &wo).rc == UKFB_ERR_INVALID_ARG);
        ukfb_weighted_out each{};
        EXPECT(!weighted_has_output(&each) && !weighted_has_output(nullptr));
        each.weight_used = &buf; EXPECT(weighted_has_output(&each));
        each = {}; each.n_used = &i32; EXPECT(weighted_has_output(&each));
    }
    return finish();
}
