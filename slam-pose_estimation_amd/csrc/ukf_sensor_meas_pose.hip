// PoseWithVelocity instantiations of the sensor-frame measurement kernel (fp64, fp32, fp32-wide)
#include "ukf_sensor_meas_launch.inc.hpp"

namespace ukfb {
int launch_sensor_meas_pose(ukfb_engine* e, const SensorReq& r) { return launch_sensor_meas_model<PoseM<double>, PoseM<float>>(e, r); }
}  // namespace ukfb
