// ukf_sensor_frame_api.hpp -- the one body behind the C-ABI of the sensor-frame measurements and of the bearing measurements
// (ukf_sensor_meas_api.hip, ukf_bearing_api.hip): the two take the same arguments and differ in the argument check
// (check_sensor_args / check_bearing_args, ukf_host.hpp) and in the kernel, which the request type names.
#pragma once

#include "ukf_api_common.hpp"
#include "ukf_feature_req.hpp"

namespace ukfb {

using SensorFrameCheck = Verdict (*)(int, bool, int, const ukfb_sensor_in*, int, const ukfb_sensor_out*);
using SensorFrameDev = int (*)(ukfb_engine*, int, const ukfb_sensor_in*, int, const ukfb_sensor_out*);

template <class Req>
int update_sensor_frame_dev(ukfb_engine* e, SensorFrameCheck check, int model_uniform, const ukfb_sensor_in* in, int commit,
                            const ukfb_sensor_out* out) {
    if (const int rc = entry(e)) return rc;
    if (const int rc = fail(check(e->model, in && in->model_dev, model_uniform, in, commit, out))) return rc;
    ON_DEVICE(e->device);
    Req r;
    r.model_uniform = model_uniform;
    r.in = *in;
    r.commit = commit != 0;
    if (out) r.out = *out;
    return launch_for_model(e, r);
}

// the host-array form: checks with `check`, stages every array given and wanted, and calls the device form `dev`
inline int update_sensor_frame(ukfb_engine* e, SensorFrameCheck check, SensorFrameDev dev, int model, const int32_t* model_per_filter,
                               const double* z, const double* Q, const double* mount, const double* mount_uniform, const double* point,
                               const double* point_uniform, int commit, double* z_pred, double* S, double* innov, double* maha,
                               double* loglik, uint32_t* status) {
    if (const int rc = entry(e)) return rc;
    // (what the device call will see: a buffer for each input given and each output wanted)
    ukfb_sensor_in in{};
    in.model_dev = model_per_filter;
    in.z_dev = z;
    in.Q_dev = Q;
    in.mount_dev = mount;
    in.point_dev = point;
    set_mount_point_uniform(&in, mount_uniform, point_uniform);
    const ukfb_sensor_out wanted{z_pred, S, innov, maha, loglik, status};
    if (const int rc = fail(check(e->model, model_per_filter != nullptr, model, &in, commit, &wanted))) return rc;
    ON_DEVICE(e->device);
    const size_t n = size_t(e->cap);
    HostStage stage(e);
    in.model_dev = stage.raw_in(model_per_filter, n);
    in.z_dev = stage.in(z, n * 3);
    in.Q_dev = stage.in(Q, n * 9);
    in.mount_dev = stage.in(mount, n * 7);
    in.point_dev = stage.in(point, n * 3);
    ukfb_sensor_out out{};
    out.z_pred = stage.out(z_pred, n * 3);
    out.S = stage.out(S, n * 9);
    out.innov = stage.out(innov, n * 3);
    out.maha = stage.out(maha, n);
    out.loglik = stage.out(loglik, n);
    out.status = stage.raw_out(status, n);
    if (const int rc = stage.rc()) return rc;
    if (const int rc = dev(e, model, &in, commit, &out)) return rc;
    return stage.finish();
}

}  // namespace ukfb
