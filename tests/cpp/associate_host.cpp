// associate_host.cpp -- the host decisions of the sensor-frame association (ukf_host.hpp) on the CPU (g++ under ASan / UBSan,
// compiled by tests/test_associate_host.py): the candidate range, NULL combinations, point_per_candidate needing point_dev,
// commit, the uniform id per engine, the order of the verdicts and the shapes of the outputs.
#include <cstdio>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

int main() {
    using namespace ukfb;
    double buf[16] = {0};
    uint32_t word = 0;
    int32_t iword = 0;
    ukfb_associate_in in{};
    in.candidates = 4;
    in.z_dev = buf;
    in.Q_dev = buf;
    in.mount_uniform[6] = 1.0;
    ukfb_associate_out none{};
    ukfb_associate_out st_only{};
    st_only.status = &word;
    const int P = UKFB_MODEL_POSE, O = UKFB_MODEL_ORIENT;
    EXPECT(UKFB_ASSOCIATE_MAX_CANDIDATES == 32 && ASSOCIATE_MAX_CANDIDATES == 32 && ASSOCIATE_MAX_CANDIDATES == MAX_CANDIDATES);
    // the candidate range: 1 ... 32, UKFB_ERR_OUT_OF_RANGE otherwise, in either mode
    for (int k = -2; k <= 40; ++k) {
        ukfb_associate_in c = in;
        c.candidates = k;
        const int want = (k >= 1 && k <= 32) ? UKFB_OK : UKFB_ERR_OUT_OF_RANGE;
        EXPECT(check_associate_args(P, false, 0, &c, 1, nullptr).rc == want);
        EXPECT(check_associate_args(O, true, 0, &c, 0, &st_only).rc == want);
        c.point_dev = buf;
        c.point_per_candidate = 1;
        EXPECT(check_associate_args(P, false, 2, &c, 1, nullptr).rc == want);
    }
    {
        ukfb_associate_in c = in;
        c.candidates = 33;
        EXPECT(check_associate_args(P, false, 0, &c, 1, nullptr).msg != nullptr);
        // the range is judged before the NULL rules, the commit flag and the model id
        c.z_dev = nullptr;
        EXPECT(check_associate_args(P, false, 7, &c, 5, nullptr).rc == UKFB_ERR_OUT_OF_RANGE);
        c.candidates = 0;
        EXPECT(check_associate_args(P, false, 7, &c, 5, nullptr).rc == UKFB_ERR_OUT_OF_RANGE);
    }
    // the uniform id is checked on the host, per-filter ids by the kernel
    for (int id = -2; id <= 9; ++id) {
        EXPECT(check_associate_args(P, false, id, &in, 1, nullptr).rc == ((id >= 0 && id <= 4) ? UKFB_OK : UKFB_ERR_WRONG_MODEL));
        EXPECT(check_associate_args(O, false, id, &in, 1, nullptr).rc == ((id >= 5 && id <= 7) ? UKFB_OK : UKFB_ERR_WRONG_MODEL));
        EXPECT(check_associate_args(P, true, id, &in, 1, nullptr).rc == UKFB_OK);
        EXPECT(check_associate_args(O, true, id, &in, 1, nullptr).rc == UKFB_OK);
    }
    EXPECT(check_associate_args(P, false, 5, &in, 1, nullptr).msg != nullptr);
    // NULL combinations
    EXPECT(check_associate_args(P, false, 0, nullptr, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
    {
        ukfb_associate_in bad = in;
        bad.z_dev = nullptr;
        EXPECT(check_associate_args(P, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad = in;
        bad.Q_dev = nullptr;
        EXPECT(check_associate_args(P, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad = in;
        bad.q_is_uniform = 2;
        EXPECT(check_associate_args(P, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad.q_is_uniform = 1;
        EXPECT(check_associate_args(P, false, 0, &bad, 1, nullptr).rc == UKFB_OK);
        bad = in;   // mount_dev / point_dev NULL: the uniform values serve; given: per filter
        bad.mount_dev = buf;
        bad.point_dev = buf;
        EXPECT(check_associate_args(P, false, 0, &bad, 1, nullptr).rc == UKFB_OK);
        // per-hypothesis mode has no uniform point: point_dev is required, whatever the model reads
        bad = in;
        bad.point_per_candidate = 1;
        EXPECT(check_associate_args(P, false, 2, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        EXPECT(check_associate_args(P, false, 3, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        EXPECT(check_associate_args(P, true, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        EXPECT(check_associate_args(P, false, 2, &bad, 1, nullptr).msg != nullptr);
        bad.point_dev = buf;
        EXPECT(check_associate_args(P, false, 2, &bad, 1, nullptr).rc == UKFB_OK);
        bad.point_per_candidate = 2;
        EXPECT(check_associate_args(P, false, 2, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad.point_per_candidate = -1;
        EXPECT(check_associate_args(P, false, 2, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
    }
    // an invalid argument is reported before a wrong model
    EXPECT(check_associate_args(P, false, 6, &in, 3, nullptr).rc == UKFB_ERR_INVALID_ARG);
    // commit is 0 or 1; a read-only call needs somewhere to write, and best / n_gated count
    EXPECT(check_associate_args(P, false, 0, &in, 2, &st_only).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_associate_args(P, false, 0, &in, -1, &st_only).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_associate_args(P, false, 0, &in, 0, nullptr).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_associate_args(P, false, 0, &in, 0, &none).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_associate_args(P, false, 0, &in, 0, &st_only).rc == UKFB_OK);
    EXPECT(check_associate_args(P, false, 0, &in, 1, &none).rc == UKFB_OK);
    {
        ukfb_associate_out o{};
        o.best = &iword;
        EXPECT(check_associate_args(O, false, 6, &in, 0, &o).rc == UKFB_OK);
        o = ukfb_associate_out{};
        o.n_gated = &iword;
        EXPECT(check_associate_args(O, false, 6, &in, 0, &o).rc == UKFB_OK);
        o = ukfb_associate_out{};
        o.S = buf;
        EXPECT(check_associate_args(O, false, 6, &in, 0, &o).rc == UKFB_OK);
    }
    // the shapes of the outputs: H hypotheses of z_pred / S, K slots of innov / maha / loglik
    for (int k = 1; k <= 32; ++k) {
        EXPECT(associate_hypotheses(k, 0) == 1 && associate_hypotheses(k, 1) == k);
        EXPECT(associate_out_scalars(associate_hypotheses(k, 1), 1022, 9) == int64_t(k) * 1022 * 9);
        EXPECT(associate_out_scalars(associate_hypotheses(k, 0), 1022, 3) == 1022 * 3);
        EXPECT(associate_out_scalars(k, 1022, 1) == int64_t(k) * 1022);
    }
    EXPECT(associate_out_scalars(32, int64_t(1) << 26, 9) == (int64_t(9) << 31));   // beyond 2^31: 64-bit
    EXPECT(associate_out_scalars(4, 0, 3) == 0);
    // the kernel borrows the sensor kernel's LDS map and launch geometry
    EXPECT(sensor_geometry(13, 12, 1022, 8).grid == 256 && sensor_geometry(14, 13, 5, 4).grid == 2 && sensor_geometry(13, 12, 0, 8).grid == 0);
    EXPECT(sensor_geometry(14, 13, 1022, 8).lds_bytes <= 65536);
    for (int id = 0; id < 8; ++id) EXPECT(sensor_reads_point(id) == (id == 1 || id == 2 || id == 6));
    return finish();
}
