// ukf_delayed_sensor_launch.hip -- typed launch of ukf_delayed_sensor_kernel<T, M, TS>: the delayed update's arguments over the
// request's window (delayed_args), then the mount, the point and the sources of the rotation rate
#include "ukf_delayed_launch.hpp"
#include "ukf_delayed_sensor.hpp"

namespace ukfb {

template <> struct FeatureLaunch<DelayedSensorReq> {
    template <class TS, class MC, class TC> static int run(ukfb_engine* e, const DelayedSensorReq& r) {
        const RowGeometry geo = delayed_sensor_geometry(MC::S, MC::D, e->cap, sizeof(TC));
        DelayedSensorArgs<TC, TS> a{};
        static_cast<DelayedArgs<TC, TS>&>(a) = delayed_args<TS, MC, TC>(e, r, r.in.model_uniform, r.in.model_dev);
        a.mount = static_cast<const TS*>(r.in.mount_dev);
        a.point = static_cast<const TS*>(r.in.point_dev);
        for (int k = 0; k < 7; ++k) a.mount_u[k] = TC(TS(r.in.mount_uniform[k]));
        for (int k = 0; k < 3; ++k) a.point_u[k] = TC(TS(r.in.point_uniform[k]));
        a.rate = static_cast<const TS*>(r.in.rate_dev);
        // (the bound rotation rate before the latched one, as the sensor-frame update reads it; no Pose model reads a rate)
        a.gyro = MC::MODEL == 1 ? static_cast<const TS*>(e->in_b_bound ? e->in_b_bound : e->in_b) : nullptr;
        return launch_rows(e, ukf_delayed_sensor_kernel<TC, MC, TS>, geo, "delayed sensor-frame kernel launch", a);
    }
};

UKFB_LAUNCH_UNIT(DelayedSensorReq)

}  // namespace ukfb
