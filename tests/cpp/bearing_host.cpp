// bearing_host.cpp -- the host decisions of the bearing measurements (ukf_host.hpp) on the CPU (g++ under ASan / UBSan, compiled
// by tests/test_bearing_host.py): model ids per engine, which inputs a model reads, NULL combinations, commit, the LDS
// accounting and the launch geometry.
#include <cstdio>

#include "../../slam-pose_estimation_amd/csrc/ukf_host.hpp"
#include "expect.hpp"

int main() {
    using namespace ukfb;
    double buf[16] = {0};
    uint32_t word = 0;
    ukfb_sensor_in in{};
    in.z_dev = buf;
    in.Q_dev = buf;
    in.mount_uniform[6] = 1.0;
    ukfb_sensor_out none{};
    ukfb_sensor_out st_only{};
    st_only.status = &word;
    // ids per engine
    EXPECT(UKFB_BEARING_NONE == -1 && UKFB_BEARING_POSE_POINT == 0 && UKFB_BEARING_POSE_NAV_DIRECTION == 1);
    EXPECT(UKFB_BEARING_ORIENT_NAV_DIRECTION == 2 && BEARING_MODELS == 3 && ROW_FILTERS_PER_GROUP == 4);
    for (int64_t id = -3; id <= 12; ++id) {
        EXPECT(bearing_model_ok(UKFB_MODEL_POSE, id) == (id == 0 || id == 1));
        EXPECT(bearing_model_ok(UKFB_MODEL_ORIENT, id) == (id == 2));
    }
    EXPECT(!bearing_model_ok(UKFB_MODEL_POSE, int64_t(1) << 40) && !bearing_model_ok(UKFB_MODEL_ORIENT, INT64_MIN));
    EXPECT(!bearing_model_ok(UKFB_MODEL_POSE, (int64_t(1) << 32) + 1) && !bearing_model_ok(UKFB_MODEL_ORIENT, (int64_t(1) << 32) + 2));
    // what a model reads: all of z and Q, qs and b; the lever arm only to a point
    for (int id = 0; id < 3; ++id) {
        int used = 0;
        for (int i = -2; i < 40; ++i) used += bearing_input_used(id, i) ? 1 : 0;
        EXPECT(used == 3 + 9 + (id == 0 ? 3 : 0) + 4 + 3);
        EXPECT(bearing_reads_lever(id) == (id == 0));
        for (int c = 0; c < 3; ++c) EXPECT(bearing_input_used(id, SENSOR_INPUT_Z + c));
        for (int k = 0; k < 9; ++k) EXPECT(bearing_input_used(id, SENSOR_INPUT_Q + k));
        for (int k = 0; k < 7; ++k) EXPECT(bearing_input_used(id, SENSOR_INPUT_MOUNT + k) == (k < 3 ? id == 0 : true));
        for (int k = 0; k < 3; ++k) EXPECT(bearing_input_used(id, SENSOR_INPUT_POINT + k));
        EXPECT(!bearing_input_used(id, SENSOR_INPUT_SCALARS) && !bearing_input_used(id, -1));
    }
    for (int id : {-1, 3, 100}) {
        EXPECT(!bearing_reads_lever(id));
        for (int i = 0; i < 32; ++i) EXPECT(!bearing_input_used(id, i));
    }
    // the uniform id is checked on the host, per-filter ids by the kernel
    for (int id = -2; id <= 9; ++id) {
        EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, id, &in, 1, nullptr).rc == ((id == 0 || id == 1) ? UKFB_OK : UKFB_ERR_WRONG_MODEL));
        EXPECT(check_bearing_args(UKFB_MODEL_ORIENT, false, id, &in, 1, nullptr).rc == (id == 2 ? UKFB_OK : UKFB_ERR_WRONG_MODEL));
        EXPECT(check_bearing_args(UKFB_MODEL_POSE, true, id, &in, 1, nullptr).rc == UKFB_OK);
        EXPECT(check_bearing_args(UKFB_MODEL_ORIENT, true, id, &in, 1, nullptr).rc == UKFB_OK);
    }
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 2, &in, 1, nullptr).msg != nullptr);
    // NULL combinations
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, nullptr, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
    {
        ukfb_sensor_in bad = in;
        bad.z_dev = nullptr;
        EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad = in;
        bad.Q_dev = nullptr;
        EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad = in;
        bad.q_is_uniform = 2;
        EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad.q_is_uniform = 1;
        EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_OK);
        bad = in;   // mount_dev / point_dev NULL: the uniform values serve; given: per filter
        bad.mount_dev = buf;
        bad.point_dev = buf;
        EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_OK);
    }
    // an invalid argument is reported before a wrong model
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 2, &in, 3, nullptr).rc == UKFB_ERR_INVALID_ARG);
    // commit is 0 or 1; a read-only call needs somewhere to write
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &in, 2, &st_only).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &in, -1, &st_only).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &in, 0, nullptr).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &in, 0, &none).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &in, 0, &st_only).rc == UKFB_OK);
    EXPECT(check_bearing_args(UKFB_MODEL_POSE, false, 0, &in, 1, &none).rc == UKFB_OK);
    {
        ukfb_sensor_out o{};
        o.S = buf;
        EXPECT(check_bearing_args(UKFB_MODEL_ORIENT, false, 2, &in, 0, &o).rc == UKFB_OK);
    }
    // LDS per model and precision: the regions of the sensor-frame kernel (the sphere side lives in registers)
    struct { int S, D; } models[2] = {{13, 12}, {14, 13}};
    for (const auto& m : models) {
        const int PK = m.D * (m.D + 1) / 2;
        const int sc = bearing_filter_scalars(m.S, m.D);
        const int floor_sc = m.D * ROW_LS + (2 * m.D + 1) * ROW_LS + m.S + PK + SENSOR_INPUT_SCALARS;
        EXPECT(sc >= floor_sc && sc <= floor_sc * 115 / 100 && sc % 4 == 0);
        EXPECT(sc == sensor_filter_scalars(m.S, m.D));
        EXPECT(2 * m.D * 4 <= (2 * m.D + 1) * ROW_LS);   // W and Y (D x 3, stride 4) fit the table they alias
        for (size_t bytes : {size_t(4), size_t(8)}) {
            const RowGeometry g = bearing_geometry(m.S, m.D, 1022, bytes);
            EXPECT(g.grid == 256 && g.lds_bytes == int(4 * sc * bytes));
            EXPECT(g.lds_bytes <= 65536 && g.lds_bytes % 16 == 0 && (sc * int(bytes)) % 16 == 0);
            EXPECT((sc * int(bytes) / 4) % 32 != 0);   // the four slices start on different banks
        }
        EXPECT(bearing_geometry(m.S, m.D, 0, 8).grid == 0 && bearing_geometry(m.S, m.D, 5, 8).grid == 2);
        EXPECT(bearing_geometry(m.S, m.D, 1, 4).grid == 1 && bearing_geometry(m.S, m.D, 4, 4).grid == 1);
    }
    EXPECT(bearing_filter_scalars(13, 12) == 676 && bearing_filter_scalars(14, 13) == 732);
    EXPECT(bearing_filter_scalars(17, 16) == -1);
    return finish();
}
