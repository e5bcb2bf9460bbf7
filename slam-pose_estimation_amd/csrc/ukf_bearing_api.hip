// ukf_bearing_api.hip -- C-ABI of the bearing measurements (include/ukf_batch.h, "bearing measurements"): the device form and
// the host-array form, over the body they share with the sensor-frame measurements.
#include "ukf_sensor_frame_api.hpp"

extern "C" {

int ukfb_update_bearing_dev(ukfb_engine* e, int model_uniform, const ukfb_sensor_in* in, int commit, const ukfb_sensor_out* out) {
    return ukfb::update_sensor_frame_dev<ukfb::BearingReq>(e, ukfb::check_bearing_args, model_uniform, in, commit, out);
}

int ukfb_update_bearing(ukfb_engine* e, int model, const int32_t* model_per_filter, const double* z, const double* Q, const double* mount,
                        const double* mount_uniform, const double* point, const double* point_uniform, int commit, double* z_pred,
                        double* S, double* innov, double* maha, double* loglik, uint32_t* status) {
    return ukfb::update_sensor_frame(e, ukfb::check_bearing_args, ukfb_update_bearing_dev, model, model_per_filter, z, Q, mount,
                                     mount_uniform, point, point_uniform, commit, z_pred, S, innov, maha, loglik, status);
}

}  // extern "C"
