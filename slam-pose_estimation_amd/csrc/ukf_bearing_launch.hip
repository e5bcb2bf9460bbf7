// ukf_bearing_launch.hip -- ukf_bearing_kernel<T, M, TS> behind the sensor-frame launch
#include "ukf_sensor_frame_launch.hpp"
#include "ukf_bearing.hpp"

namespace ukfb {

template <> struct SensorFrameKernel<true> {
    template <class TC, class MC, class TS> static constexpr auto kernel = ukf_bearing_kernel<TC, MC, TS>;
    static constexpr const char* what = "bearing kernel launch";
    static constexpr bool gyro = false;   // (no bearing model reads the latched rotation rate)
};

UKFB_LAUNCH_UNIT(BearingReq)

}  // namespace ukfb
