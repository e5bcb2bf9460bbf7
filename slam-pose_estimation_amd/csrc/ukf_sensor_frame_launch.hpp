// ukf_sensor_frame_launch.hpp -- the one typed launch of the sensor-frame measurement kernels: ukf_sensor_meas_kernel and
// ukf_bearing_kernel<T, M, TS> take the same SensorArgs over the same LDS map.  A launch source names its kernel by
// specialising SensorFrameKernel<BEARING>.
#pragma once

#include "ukf_feature_launch.hpp"
#include "ukf_feature_req.hpp"
#include "ukf_sensor_meas.hpp"

namespace ukfb {

// template <class TC, class MC, class TS> static constexpr auto kernel; static constexpr const char* what;
// static constexpr bool gyro: a model of the kernel reads the latched rotation rate
template <bool BEARING> struct SensorFrameKernel;

template <bool BEARING> struct FeatureLaunch<SensorFrameReq<BEARING>> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const SensorFrameReq<BEARING>& r) {
        using K = SensorFrameKernel<BEARING>;
        const RowGeometry geo = sensor_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        SensorArgs<TC, TS> a{};
        bind_state<TS>(a, e, r.commit);
        bind_sensor_inputs<TS, TC>(a, e, r, K::gyro);
        bind_mean<TS, TC>(a, e);
        bind_gate<TS, TC>(a, e);
        return launch_rows(e, K::template kernel<TC, MC, TS>, geo, K::what, a);
    }
};

}  // namespace ukfb
