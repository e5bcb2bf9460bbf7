// ukf_sensor_meas_launch.hip -- ukf_sensor_meas_kernel<T, M, TS> behind the sensor-frame launch
#include "ukf_sensor_frame_launch.hpp"

namespace ukfb {

template <> struct SensorFrameKernel<false> {
    template <class TC, class MC, class TS> static constexpr auto kernel = ukf_sensor_meas_kernel<TC, MC, TS>;
    static constexpr const char* what = "sensor-measurement kernel launch";
    static constexpr bool gyro = true;
};

UKFB_LAUNCH_UNIT(SensorReq)

}  // namespace ukfb
