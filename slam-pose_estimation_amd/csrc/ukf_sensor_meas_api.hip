// ukf_sensor_meas_api.hip -- C-ABI of the sensor-frame measurements (include/ukf_batch.h, "sensor-frame measurements"): the
// device form and the host-array form, over the body they share with the bearing measurements.
#include "ukf_sensor_frame_api.hpp"

extern "C" {

int ukfb_update_sensor_dev(ukfb_engine* e, int model_uniform, const ukfb_sensor_in* in, int commit, const ukfb_sensor_out* out) {
    return ukfb::update_sensor_frame_dev<ukfb::SensorReq>(e, ukfb::check_sensor_args, model_uniform, in, commit, out);
}

int ukfb_update_sensor(ukfb_engine* e, int model, const int32_t* model_per_filter, const double* z, const double* Q, const double* mount,
                       const double* mount_uniform, const double* point, const double* point_uniform, int commit, double* z_pred,
                       double* S, double* innov, double* maha, double* loglik, uint32_t* status) {
    return ukfb::update_sensor_frame(e, ukfb::check_sensor_args, ukfb_update_sensor_dev, model, model_per_filter, z, Q, mount, mount_uniform,
                                     point, point_uniform, commit, z_pred, S, innov, maha, loglik, status);
}

}  // extern "C"
