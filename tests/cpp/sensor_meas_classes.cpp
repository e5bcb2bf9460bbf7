// sensor_meas_classes.cpp -- integrateSensorMeasurement of include/pose_estimation/Batch.hpp from a C++ host (compiled and run by
// tests/test_gpu_sensor_meas.py): reads a batch's state and one uniform sensor-frame measurement from a file of doubles, applies
// it, and writes the new state and every output back, so that the test can compare the bits with the device form's.
//   in : int64 n, model (0 Pose / 1 OrientationState), sensor model id; then doubles mu [n][S], cov [n][D][D], gyro [n][3],
//        z [n][3], Q [n][3][3], mount [7], point [3]
//   out: doubles mu, cov, z_pred [n][3], S [n][3][3], innov [n][3], maha [n], loglik [n], status [n]
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "pose_estimation/Batch.hpp"

static std::vector<double> take(std::FILE* f, size_t count) {
    std::vector<double> v(count);
    if (count && std::fread(v.data(), sizeof(double), count, f) != count) throw std::runtime_error("short input file");
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) throw std::runtime_error("cannot open the input file");
        int64_t head[3];
        if (std::fread(head, sizeof(int64_t), 3, f) != 3) throw std::runtime_error("short input file");
        const size_t n = size_t(head[0]);
        const bool pose = head[1] == 0;
        const size_t S = pose ? 13 : 14, D = pose ? 12 : 13;
        const std::vector<double> mu = take(f, n * S), cov = take(f, n * D * D), gyro = take(f, n * 3), z = take(f, n * 3),
                                  Q = take(f, n * 9), mount = take(f, 7), point = take(f, 3);
        std::fclose(f);
        std::vector<double> mu_o(n * S), cov_o(n * D * D), z_pred(n * 3), Sm(n * 9), innov(n * 3), maha(n), loglik(n);
        std::vector<uint32_t> st;
        const double earth[3] = {0.0, 0.0, 0.0};
        pose_estimation::BatchPoseUKF* pe = pose ? new pose_estimation::BatchPoseUKF(int64_t(n)) : NULL;
        pose_estimation::BatchOrientationUKF* oe = pose ? NULL : new pose_estimation::BatchOrientationUKF(int64_t(n), 3600.0, 3600.0, earth);
        pose_estimation::BatchUKF* e = pose ? static_cast<pose_estimation::BatchUKF*>(pe) : oe;
        e->initializeFilters(0, int64_t(n), mu.data(), cov.data());
        if (oe) oe->setInputs(0, int64_t(n), gyro.data(), NULL);
        st = e->integrateSensorMeasurement(int(head[2]), z.data(), Q.data(), mount.data(), point.data(), NULL, NULL, NULL, true,
                                           z_pred.data(), Sm.data(), innov.data(), maha.data(), loglik.data());
        e->getCurrentStates(0, int64_t(n), mu_o.data(), cov_o.data());
        delete pe;
        delete oe;
        std::FILE* o = std::fopen(argv[2], "wb");
        if (!o) throw std::runtime_error("cannot open the output file");
        const std::vector<double> status(st.begin(), st.end());
        const std::vector<double>* parts[] = {&mu_o, &cov_o, &z_pred, &Sm, &innov, &maha, &loglik, &status};
        for (const std::vector<double>* p : parts)
            if (std::fwrite(p->data(), sizeof(double), p->size(), o) != p->size()) throw std::runtime_error("short write");
        std::fclose(o);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "sensor_meas_classes: %s\n", ex.what());
        return 1;
    }
    return 0;
}
