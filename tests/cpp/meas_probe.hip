// Test helper: evaluates the shipped measurement-side primitives of the sensor-frame, bearing, association and sampled kernels
// -- s2_log, s2_exp, bearing_h (ukf_bearing.hpp), cos_sinc_sqrt (ukf_device.hpp), sensor_h, sensor_solve3 (ukf_sensor_meas.hpp)
// and sampled_solve6 (ukf_sampled.hpp) -- one record per lane, so that tests/test_gpu_meas_primitives.py can hold each of them
// against a 40-digit reference at its regime edges and check that a lane's result does not depend on the other lanes of its
// wavefront (s2_log has a wave vote, sensor_h skips rotations by wave-uniform flags).
//
// Records: MEASP_IN doubles in, MEASP_OUT doubles out, layout per primitive in the table below.  The sphere maps and the models
// are the fp64 instantiations the kernels ship; cos_sinc_sqrt and the solves run in T: inputs are converted to T (the caller
// passes values that are exact in T) and the results are widened back to double.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../slam-pose_estimation_amd/csrc/ukf_bearing.hpp"
#include "../../slam-pose_estimation_amd/csrc/ukf_sampled.hpp"

enum { MEASP_IN = 33, MEASP_OUT = 6 };
// the model records: x[S] from 0, then
enum { MR_ID = 14, MR_R = 15, MR_QSI = 18, MR_B = 22, MR_GY = 25, MR_RNQ = 28 };

// primitive ids (tests/meas_primitives_reference.py PRIM)
enum {
    P_S2_LOG = 0,          // u[3], v[3]                                              -> w[3]
    P_S2_EXP = 1,          // u[3], w[3]                                              -> r[3]
    P_COS_SINC_SQRT = 2,   // x2                                                      -> cos, sinc          (T)
    P_BEARING_POSE = 3,    // x[13], [14] to_point, r[3], qsi[4], b[3], [28] rnq      -> z[3], flag
    P_BEARING_ORIENT = 4,  // x[14],                r[3], qsi[4], b[3], [28] rnq      -> z[3], flag
    P_SENSOR_POSE = 5,     // x[13], [14] id 0..4,  r[3], qsi[4], b[3], [28] rnq      -> z[3]
    P_SENSOR_ORIENT = 6,   // x[14], [14] id 5..7,  r[3], qsi[4], b[3], gy[3], [28] rnq -> z[3]
    P_SOLVE3 = 7,          // c[3], l10, l20, l21, rs[3]                              -> c[3]               (T)
    P_SOLVE6 = 8,          // c[6], lf[21], rs[6]; m is the kernel argument           -> c[6]               (T)
    P_COUNT
};

template <class T> __global__ void __launch_bounds__(256) meas_probe_kernel(int prim, int m, int64_t n, const double* in, double* out) {
    using namespace ukfb;
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    // lanes past the end evaluate the last record (every lane of a wavefront takes part in the votes) and store nothing
    const int64_t j = i < n ? i : n - 1;
    double a[MEASP_IN];
#pragma unroll
    for (int k = 0; k < MEASP_IN; ++k) a[k] = in[j * MEASP_IN + k];
    double r[MEASP_OUT];
#pragma unroll
    for (int k = 0; k < MEASP_OUT; ++k) r[k] = 0.0;
    switch (prim) {   // kernel argument: wave-uniform
    case P_S2_LOG:
    case P_S2_EXP: {
        const double u[3] = {a[0], a[1], a[2]}, v[3] = {a[3], a[4], a[5]};
        double w[3];
        if (prim == P_S2_LOG) s2_log(u, v, w);
        else s2_exp(u, v, w);
        r[0] = w[0]; r[1] = w[1]; r[2] = w[2];
        break;
    }
    case P_COS_SINC_SQRT: {
        T c, s;
        cos_sinc_sqrt(T(a[0]), c, s);
        r[0] = double(c); r[1] = double(s);
        break;
    }
    case P_BEARING_POSE:
    case P_BEARING_ORIENT: {
        BearingIn hin;
#pragma unroll
        for (int k = 0; k < 3; ++k) { hin.r[k] = a[MR_R + k]; hin.b[k] = a[MR_B + k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) hin.qsi[k] = a[MR_QSI + k];
        hin.rnq = a[MR_RNQ];
        double z[3];
        bool ok;
        if (prim == P_BEARING_POSE) {
            double x[13];
#pragma unroll
            for (int k = 0; k < 13; ++k) x[k] = a[k];
            ok = bearing_h<PoseM<double>>(x, a[MR_ID] != 0.0, hin, z);
        } else {
            double x[14];
#pragma unroll
            for (int k = 0; k < 14; ++k) x[k] = a[k];
            ok = bearing_h<OrientM<double>>(x, false, hin, z);
        }
        r[0] = z[0]; r[1] = z[1]; r[2] = z[2]; r[3] = ok ? 1.0 : 0.0;
        break;
    }
    case P_SENSOR_POSE:
    case P_SENSOR_ORIENT: {
        SensorIn<double> hin;
#pragma unroll
        for (int k = 0; k < 3; ++k) { hin.r[k] = a[MR_R + k]; hin.b[k] = a[MR_B + k]; hin.gy[k] = a[MR_GY + k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) hin.qsi[k] = a[MR_QSI + k];
        hin.rnq = a[MR_RNQ];
        const int id = int(a[MR_ID]);
        // the flags as the kernels form them (ukf_sensor_meas.hpp, ukf_associate.hpp): votes over the wavefront's ids
        const bool need_sens = wave_any(sensor_reads_rotation(int64_t(id)));
        const bool need_point = wave_any(id == UKFB_SENSOR_POSE_POINT);
        const bool need_fwd = wave_any(id == UKFB_SENSOR_POSE_POSITION || id == UKFB_SENSOR_POSE_RANGE || id == UKFB_SENSOR_POSE_NAV_VELOCITY);
        double z[3];
        if (prim == P_SENSOR_POSE) {
            double x[13];
#pragma unroll
            for (int k = 0; k < 13; ++k) x[k] = a[k];
            sensor_h((PoseM<double>*)nullptr, x, id, hin, need_fwd, need_point, need_sens, z);
        } else {
            double x[14];
#pragma unroll
            for (int k = 0; k < 14; ++k) x[k] = a[k];
            sensor_h((OrientM<double>*)nullptr, x, id, hin, need_fwd, need_point, need_sens, z);
        }
        r[0] = z[0]; r[1] = z[1]; r[2] = z[2];
        break;
    }
    case P_SOLVE3: {
        T c[3] = {T(a[0]), T(a[1]), T(a[2])};
        const T rs[3] = {T(a[6]), T(a[7]), T(a[8])};
        sensor_solve3(c, T(a[3]), T(a[4]), T(a[5]), rs);
        r[0] = double(c[0]); r[1] = double(c[1]); r[2] = double(c[2]);
        break;
    }
    case P_SOLVE6: {
        T c[SAMPLED_MAX_M], lf[21], rs[SAMPLED_MAX_M];
#pragma unroll
        for (int k = 0; k < SAMPLED_MAX_M; ++k) { c[k] = T(a[k]); rs[k] = T(a[SAMPLED_MAX_M + 21 + k]); }
#pragma unroll
        for (int k = 0; k < 21; ++k) lf[k] = T(a[SAMPLED_MAX_M + k]);
        sampled_solve6(c, lf, rs, m);
#pragma unroll
        for (int k = 0; k < SAMPLED_MAX_M; ++k) r[k] = double(c[k]);
        break;
    }
    default: break;
    }
    if (i < n) {
#pragma unroll
        for (int k = 0; k < MEASP_OUT; ++k) out[i * MEASP_OUT + k] = r[k];
    }
}

// prec 0: double, 1: float (cos_sinc_sqrt and the solves only).  m: sampled_solve6's dimension, 1 ... 6.  Returns 0 on success.
extern "C" int meas_probe(int prim, int prec, int m, int64_t n, const double* in, double* out) {
    static_assert(ukfb::SAMPLED_MAX_M == 6 && MEASP_IN >= 2 * ukfb::SAMPLED_MAX_M + 21 && MEASP_OUT >= ukfb::SAMPLED_MAX_M, "a solve6 record fits");
    const bool in_t = prim == P_COS_SINC_SQRT || prim == P_SOLVE3 || prim == P_SOLVE6;
    if (prim < 0 || prim >= P_COUNT || (prec != 0 && prec != 1) || (prec == 1 && !in_t) || n <= 0 || !in || !out) return 1;
    if (prim == P_SOLVE6 && (m < 1 || m > ukfb::SAMPLED_MAX_M)) return 1;
    double *d_in = nullptr, *d_out = nullptr;
    const size_t bin = size_t(n) * MEASP_IN * sizeof(double), bout = size_t(n) * MEASP_OUT * sizeof(double);
    if (hipMalloc(reinterpret_cast<void**>(&d_in), bin) != hipSuccess) return 2;
    if (hipMalloc(reinterpret_cast<void**>(&d_out), bout) != hipSuccess) {
        (void)hipFree(d_in);
        return 2;
    }
    int rc = 0;
    if (hipMemcpy(d_in, in, bin, hipMemcpyHostToDevice) != hipSuccess) rc = 3;
    if (!rc) {
        const dim3 block(256), grid(unsigned((n + 255) / 256));
        if (prec == 0) hipLaunchKernelGGL(meas_probe_kernel<double>, grid, block, 0, 0, prim, m, n, d_in, d_out);
        else hipLaunchKernelGGL(meas_probe_kernel<float>, grid, block, 0, 0, prim, m, n, d_in, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 4;
    }
    if (!rc && hipMemcpy(out, d_out, bout, hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}
