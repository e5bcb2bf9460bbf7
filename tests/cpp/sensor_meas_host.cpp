// sensor_meas_host.cpp -- the host decisions of the sensor-frame measurements (ukf_host.hpp) on the CPU (g++ under ASan / UBSan,
// compiled by tests/test_sensor_meas_host.py): model ids per engine, the measurement dimension, which inputs a model reads,
// NULL combinations, commit, and the launch geometry.
#include <cstdio>
#include <vector>

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
    EXPECT(UKFB_SENSOR_POSE_POSITION == 0 && UKFB_SENSOR_POSE_RANGE == 1 && UKFB_SENSOR_POSE_POINT == 2 && UKFB_SENSOR_POSE_VELOCITY == 3);
    EXPECT(UKFB_SENSOR_POSE_NAV_VELOCITY == 4 && UKFB_SENSOR_ORIENT_VELOCITY == 5 && UKFB_SENSOR_ORIENT_NAV_VECTOR == 6);
    EXPECT(UKFB_SENSOR_ORIENT_SPECIFIC_FORCE == 7 && UKFB_SENSOR_NONE == -1 && SENSOR_MODELS == 8);
    for (int64_t id = -3; id <= 12; ++id) {
        EXPECT(sensor_model_ok(UKFB_MODEL_POSE, id) == (id >= 0 && id <= 4));
        EXPECT(sensor_model_ok(UKFB_MODEL_ORIENT, id) == (id >= 5 && id <= 7));
        EXPECT(sensor_meas_dim(id) == ((id < 0 || id > 7) ? 0 : (id == 1 ? 1 : 3)));
    }
    EXPECT(!sensor_model_ok(UKFB_MODEL_POSE, int64_t(1) << 40) && !sensor_model_ok(UKFB_MODEL_ORIENT, INT64_MIN));
    // which of mount / point a model reads: the table of include/ukf_batch.h
    const bool lever[8] = {true, true, true, true, false, true, false, false};
    const bool rotation[8] = {false, false, true, true, false, true, true, false};
    const bool point[8] = {false, true, true, false, false, false, true, false};
    for (int id = 0; id < 8; ++id) {
        EXPECT(sensor_reads_lever(id) == lever[id] && sensor_reads_rotation(id) == rotation[id] && sensor_reads_point(id) == point[id]);
        const int m = sensor_meas_dim(id);
        int used = 0;
        for (int i = -2; i < 40; ++i) used += sensor_input_used(id, i) ? 1 : 0;
        EXPECT(used == m + m * m + (lever[id] ? 3 : 0) + (rotation[id] ? 4 : 0) + (point[id] ? 3 : 0));
        for (int c = 0; c < 3; ++c) EXPECT(sensor_input_used(id, SENSOR_INPUT_Z + c) == (c < m));
        for (int k = 0; k < 9; ++k) EXPECT(sensor_input_used(id, SENSOR_INPUT_Q + k) == (k / 3 < m && k % 3 < m));
        for (int k = 0; k < 7; ++k) EXPECT(sensor_input_used(id, SENSOR_INPUT_MOUNT + k) == (k < 3 ? lever[id] : rotation[id]));
        for (int k = 0; k < 3; ++k) EXPECT(sensor_input_used(id, SENSOR_INPUT_POINT + k) == point[id]);
    }
    for (int id : {-1, 8, 100}) {
        EXPECT(!sensor_reads_lever(id) && !sensor_reads_rotation(id) && !sensor_reads_point(id));
        for (int i = 0; i < 32; ++i) EXPECT(!sensor_input_used(id, i));
    }
    EXPECT(SENSOR_INPUT_SCALARS == 22 && SENSOR_INPUT_POINT + 3 == SENSOR_INPUT_SCALARS);
    for (int i = 0; i < 32; ++i) EXPECT(sensor_input_neutral(i) == (i == 18 ? 1.0 : 0.0));   // qs = (0, 0, 0, 1)
    // the uniform id is checked on the host, per-filter ids by the kernel
    for (int id = -2; id <= 9; ++id) {
        EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, id, &in, 1, nullptr).rc == ((id >= 0 && id <= 4) ? UKFB_OK : UKFB_ERR_WRONG_MODEL));
        EXPECT(check_sensor_args(UKFB_MODEL_ORIENT, false, id, &in, 1, nullptr).rc == ((id >= 5 && id <= 7) ? UKFB_OK : UKFB_ERR_WRONG_MODEL));
        EXPECT(check_sensor_args(UKFB_MODEL_POSE, true, id, &in, 1, nullptr).rc == UKFB_OK);
    }
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 5, &in, 1, nullptr).msg != nullptr);
    // NULL combinations
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, nullptr, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
    {
        ukfb_sensor_in bad = in;
        bad.z_dev = nullptr;
        EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad = in;
        bad.Q_dev = nullptr;
        EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad = in;
        bad.q_is_uniform = 2;
        EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_ERR_INVALID_ARG);
        bad.q_is_uniform = 1;
        EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &bad, 1, nullptr).rc == UKFB_OK);
        bad = in;   // mount_dev / point_dev NULL: the uniform values serve; given: per filter
        bad.mount_dev = buf;
        bad.point_dev = buf;
        EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 2, &bad, 1, nullptr).rc == UKFB_OK);
    }
    // an invalid argument is reported before a wrong model
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 7, &in, 3, nullptr).rc == UKFB_ERR_INVALID_ARG);
    // commit is 0 or 1; a read-only call needs somewhere to write
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &in, 2, &st_only).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &in, -1, &st_only).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &in, 0, nullptr).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &in, 0, &none).rc == UKFB_ERR_INVALID_ARG);
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &in, 0, &st_only).rc == UKFB_OK);
    EXPECT(check_sensor_args(UKFB_MODEL_POSE, false, 0, &in, 1, &none).rc == UKFB_OK);
    {
        ukfb_sensor_out o{};
        o.z_pred = buf;
        EXPECT(check_sensor_args(UKFB_MODEL_ORIENT, false, 6, &in, 0, &o).rc == UKFB_OK);
    }
    // LDS per model and precision: four filters per workgroup, lighter than the state-measurement kernel
    struct { int S, D; } models[2] = {{13, 12}, {14, 13}};
    for (const auto& m : models) {
        const int PK = m.D * (m.D + 1) / 2;
        const int sc = sensor_filter_scalars(m.S, m.D);
        // one D x 14 matrix, the commit's delta table, one record, the inputs, and no more than 15 % on top
        const int floor_sc = m.D * ROW_LS + (2 * m.D + 1) * ROW_LS + m.S + PK + SENSOR_INPUT_SCALARS;
        EXPECT(sc >= floor_sc && sc <= floor_sc * 115 / 100 && sc % 4 == 0);
        EXPECT(sc < state_meas_filter_scalars(m.S, m.D));
        EXPECT(2 * m.D * 4 <= (2 * m.D + 1) * ROW_LS);   // W and Y (D x 3, stride 4) fit the table they alias
        for (size_t bytes : {size_t(4), size_t(8)}) {
            const RowGeometry g = sensor_geometry(m.S, m.D, 1022, bytes);
            EXPECT(g.grid == 256 && g.lds_bytes == int(4 * sc * bytes));
            EXPECT(g.lds_bytes <= 65536 && g.lds_bytes % 16 == 0 && (sc * int(bytes)) % 16 == 0);
            EXPECT((sc * int(bytes) / 4) % 32 != 0);   // the four slices start on different banks
        }
        EXPECT(sensor_geometry(m.S, m.D, 0, 8).grid == 0 && sensor_geometry(m.S, m.D, 5, 8).grid == 2);
        EXPECT(sensor_geometry(m.S, m.D, 1, 4).grid == 1 && sensor_geometry(m.S, m.D, 4, 4).grid == 1);
    }
    EXPECT(sensor_filter_scalars(13, 12) == 676 && sensor_filter_scalars(14, 13) == 732);
    EXPECT(sensor_filter_scalars(17, 16) == -1);
    return finish();
}
