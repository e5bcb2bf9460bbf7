// feature_launch_host.cpp -- the host half of the feature launches (ukf_feature_bind.hpp) on the CPU (g++ under ASan / UBSan,
// compiled by tests/test_feature_launch_host.py; no HIP is linked): the choice of precision and model, the commit rule, the
// process block with the precedence of its inputs, the rounding of every scalar through the storage type (against the
// expressions of the launches before they shared a binder, written out here), and the sensor-frame inputs.  The engine is a plain
// ukfb_engine whose pointers are host addresses that nobody dereferences.
#include <cstring>
#include <type_traits>

#include "../../slam-pose_estimation_amd/csrc/ukf_feature_bind.hpp"
#include "expect.hpp"

// the members the binders name, in no kernel's order
template <class T, class TS> struct Args {
    int64_t n;
    const TS *mu, *cov;
    TS *mu_out, *cov_out, *eng_mu, *eng_cov;
    uint32_t* engine_status;
    const uint8_t* initialised;
    const TS *Rn, *Racc, *in_a, *in_b;
    int64_t Rn_stride;
    int in_ring, mean_max_it;
    T ninv_tau_g, ninv_tau_a, earth[3], mean_tol, gate_chi2;
    double min_dt, max_dt;
    int model_uniform, q_uniform;
    const int32_t* model;
    const TS *z, *Q, *mount, *point, *gyro;
    T mount_u[7], point_u[3];
    TS *z_pred, *S, *innov, *maha, *loglik;
    uint32_t* status;
};

struct SensorLikeReq {
    int model_uniform = -1;
    ukfb_sensor_in in{};
    ukfb_sensor_out out{};
};

struct DummyReq {
    int tag;
};
struct PoseOnlyReq {
    int tag;
};
struct M64 {};
struct M32 {};

namespace ukfb {
template <class Req> int launch_pose(ukfb_engine*, const Req& r) { return 100 + r.tag; }
template <class Req> int launch_orient(ukfb_engine*, const Req& r) { return 200 + r.tag; }
template <> inline constexpr bool pose_only<PoseOnlyReq> = true;
}  // namespace ukfb

template <class T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// addresses to tell apart
static unsigned char arena[32];
static void* at(int k) { return arena + k; }

static ukfb_engine make_engine() {
    ukfb_engine e;
    e.model = UKFB_MODEL_POSE;
    e.prec = UKFB_F64;
    e.cap = 7;
    e.mu = at(1);
    e.cov = at(2);
    e.status = reinterpret_cast<uint32_t*>(at(3));
    e.init = reinterpret_cast<uint8_t*>(at(4));
    e.Rn = at(5);
    e.Racc = at(6);
    e.in_a = at(7);
    e.in_b = at(8);
    // values whose float and double roundings differ
    e.tau_g = 3.0;
    e.tau_a = 7.0;
    e.earth[0] = 7.292115e-5;
    e.earth[1] = 1e-9;
    e.earth[2] = 0.1;
    e.cfg.mean_tol = 1e-9;
    e.cfg.mean_max_iter = 37;
    e.cfg.gate_chi2 = 7.815;
    e.cfg.min_time_delta = 1e-7;
    e.cfg.max_time_delta = 2.5;
    return e;
}

static void check_precision_choice() {
    ukfb_engine e = make_engine();
    // 1: (double, M64, double), 2: (float, M32, double), 3: (float, M32, float), 0: anything else
    const auto which = [](auto p) {
        using P = decltype(p);
        const bool m64 = std::is_same<typename P::M, M64>::value, m32 = std::is_same<typename P::M, M32>::value;
        const bool sd = std::is_same<typename P::TS, double>::value, sf = std::is_same<typename P::TS, float>::value;
        const bool cd = std::is_same<typename P::TC, double>::value, cf = std::is_same<typename P::TC, float>::value;
        return (sd && cd && m64) ? 1 : (sf && cd && m32) ? 2 : (sf && cf && m32) ? 3 : 0;
    };
    e.prec = UKFB_F64;
    e.cfg.wide_arithmetic = 0;
    EXPECT((ukfb::dispatch_precision<M64, M32>(&e, which) == 1));
    e.cfg.wide_arithmetic = 1;   // (has no meaning for an fp64 engine)
    EXPECT((ukfb::dispatch_precision<M64, M32>(&e, which) == 1));
    e.prec = UKFB_F32;
    EXPECT((ukfb::dispatch_precision<M64, M32>(&e, which) == 2));
    e.cfg.wide_arithmetic = 0;
    EXPECT((ukfb::dispatch_precision<M64, M32>(&e, which) == 3));
}

static void check_model_dispatch() {
    ukfb_engine e = make_engine();
    e.model = UKFB_MODEL_POSE;
    EXPECT(ukfb::launch_for_model(&e, DummyReq{5}) == 105);
    EXPECT(ukfb::launch_for_model(&e, PoseOnlyReq{6}) == 106);
    e.model = UKFB_MODEL_ORIENT;
    EXPECT(ukfb::launch_for_model(&e, DummyReq{5}) == 205);
    EXPECT(ukfb::launch_for_model(&e, PoseOnlyReq{6}) == 106);   // (its check refuses the engine before; no Orient launch exists)
}

template <class TS, class TC> static void check_binders() {
    using A = Args<TC, TS>;
    ukfb_engine e = make_engine();

    // ---- commit
    {
        A a{};
        ukfb::bind_state<TS>(a, &e, false);
        EXPECT(a.mu_out == nullptr && a.cov_out == nullptr && a.engine_status == nullptr);
        EXPECT(a.n == 7 && a.mu == e.mu && a.cov == e.cov && a.initialised == e.init);
        A b{};
        ukfb::bind_state<TS>(b, &e, true);
        EXPECT(b.mu_out == e.mu && b.cov_out == e.cov && b.engine_status == e.status);
        EXPECT(b.n == 7 && b.mu == e.mu && b.cov == e.cov && b.initialised == e.init);
        // the form for a struct whose mu_out / cov_out are the caller's: they are left alone
        A c{};
        c.mu_out = static_cast<TS*>(at(20));
        ukfb::bind_state<TS>(c, &e, false, c.eng_mu, c.eng_cov);
        EXPECT(c.eng_mu == nullptr && c.eng_cov == nullptr && c.engine_status == nullptr && c.mu_out == at(20) && c.mu == e.mu);
        ukfb::bind_state<TS>(c, &e, true, c.eng_mu, c.eng_cov);
        EXPECT(c.eng_mu == e.mu && c.eng_cov == e.cov && c.engine_status == e.status && c.mu_out == at(20) && c.cov_out == nullptr);
        // the commit half alone
        A d{};
        ukfb::bind_commit<TS>(d, &e, false);
        EXPECT(d.mu_out == nullptr && d.cov_out == nullptr && d.engine_status == nullptr && d.mu == nullptr && d.n == 0);
        ukfb::bind_commit<TS>(d, &e, true);
        EXPECT(d.mu_out == e.mu && d.cov_out == e.cov && d.engine_status == e.status && d.mu == nullptr);
    }

    // ---- process block: noise stride, precedence of the inputs, ring bits
    {
        A a{};
        e.Rn_per_filter = false;
        ukfb::bind_process<TS, TC>(a, &e, 12, nullptr, nullptr);
        EXPECT(a.Rn_stride == 0 && a.Rn == e.Rn && a.Racc == e.Racc);
        EXPECT(a.in_a == e.in_a && a.in_b == e.in_b && a.in_ring == 0);   // latched
        EXPECT(a.mean_max_it == 37 && a.min_dt == 1e-7 && a.max_dt == 2.5);
        e.Rn_per_filter = true;
        ukfb::bind_process<TS, TC>(a, &e, 12, nullptr, nullptr);
        EXPECT(a.Rn_stride == 144);
        ukfb::bind_process<TS, TC>(a, &e, 13, nullptr, nullptr);
        EXPECT(a.Rn_stride == 169);
        e.in_a_bound = at(9);
        e.in_b_bound = at(10);
        ukfb::bind_process<TS, TC>(a, &e, 12, nullptr, nullptr);
        EXPECT(a.in_a == at(9) && a.in_b == at(10) && a.in_ring == 0);   // bound before latched
        ukfb::bind_process<TS, TC>(a, &e, 12, at(11), nullptr);
        EXPECT(a.in_a == at(11) && a.in_b == at(10) && a.in_ring == 1);   // the request's ring before bound
        ukfb::bind_process<TS, TC>(a, &e, 12, nullptr, at(12));
        EXPECT(a.in_a == at(9) && a.in_b == at(12) && a.in_ring == 2);
        ukfb::bind_process<TS, TC>(a, &e, 12, at(11), at(12));
        EXPECT(a.in_a == at(11) && a.in_b == at(12) && a.in_ring == 3);
        e.in_a_bound = e.in_b_bound = nullptr;
        ukfb::bind_process<TS, TC>(a, &e, 12, at(11), nullptr);
        EXPECT(a.in_a == at(11) && a.in_b == e.in_b && a.in_ring == 1);   // the ring before latched
    }

    // ---- rounding: the expressions of the launches before the binders, literally
    {
        A a{};
        ukfb::bind_process<TS, TC>(a, &e, 12, nullptr, nullptr);
        EXPECT(same_bits<TC>(a.ninv_tau_g, TC(TS(-1.0) / TS(e.tau_g))));
        EXPECT(same_bits<TC>(a.ninv_tau_a, TC(TS(-1.0) / TS(e.tau_a))));
        for (int k = 0; k < 3; ++k) EXPECT(same_bits<TC>(a.earth[k], TC(TS(e.earth[k]))));
        EXPECT(same_bits<TC>(a.mean_tol, TC(TS(e.cfg.mean_tol))));
        A b{};
        ukfb::bind_mean<TS, TC>(b, &e);
        ukfb::bind_gate<TS, TC>(b, &e);
        EXPECT(same_bits<TC>(b.mean_tol, TC(TS(e.cfg.mean_tol))) && b.mean_max_it == 37);
        EXPECT(same_bits<TC>(b.gate_chi2, TC(TS(e.cfg.gate_chi2))));
        // a storage type narrower than the compute type shows in the value: the double is the float's, not the engine's own
        if (!std::is_same<TS, TC>::value) {
            EXPECT(double(a.ninv_tau_g) != -1.0 / 3.0 && double(a.earth[0]) != e.earth[0] && double(b.mean_tol) != 1e-9 &&
                   double(b.gate_chi2) != 7.815);
            EXPECT(double(a.ninv_tau_g) == double(-1.0f / 3.0f) && double(b.gate_chi2) == double(7.815f));
        }
        if (std::is_same<TS, double>::value) EXPECT(double(a.ninv_tau_g) == -1.0 / 3.0 && double(b.mean_tol) == 1e-9);
    }

    // ---- sensor-frame inputs
    {
        SensorLikeReq r;
        r.model_uniform = 4;
        r.in.model_dev = reinterpret_cast<const int32_t*>(at(13));
        r.in.z_dev = at(14);
        r.in.Q_dev = at(15);
        r.in.q_is_uniform = 1;
        r.in.mount_dev = at(16);
        r.in.point_dev = at(17);
        for (int k = 0; k < 7; ++k) r.in.mount_uniform[k] = 0.1 * (k + 1) + 1e-9;
        for (int k = 0; k < 3; ++k) r.in.point_uniform[k] = 1.0 / (k + 3);
        r.out = ukfb_sensor_out{at(21), at(22), at(23), at(24), at(25), reinterpret_cast<uint32_t*>(at(26))};
        A a{};
        ukfb::bind_sensor_inputs<TS, TC>(a, &e, r, true);
        EXPECT(a.model_uniform == 4 && a.model == r.in.model_dev && a.z == at(14) && a.Q == at(15) && a.q_uniform == 1);
        EXPECT(a.mount == at(16) && a.point == at(17));
        EXPECT(a.z_pred == at(21) && a.S == at(22) && a.innov == at(23) && a.maha == at(24) && a.loglik == at(25) && a.status == r.out.status);
        for (int k = 0; k < 7; ++k) EXPECT(same_bits<TC>(a.mount_u[k], TC(TS(r.in.mount_uniform[k]))));
        for (int k = 0; k < 3; ++k) EXPECT(same_bits<TC>(a.point_u[k], TC(TS(r.in.point_uniform[k]))));
        if (!std::is_same<TS, TC>::value) EXPECT(double(a.mount_u[0]) != r.in.mount_uniform[0] && double(a.point_u[0]) != r.in.point_uniform[0]);
        EXPECT(a.gyro == e.in_b);   // the sensor form: latched
        e.in_b_bound = at(10);
        ukfb::bind_sensor_inputs<TS, TC>(a, &e, r, true);
        EXPECT(a.gyro == at(10));   // bound before latched
        ukfb::bind_sensor_inputs<TS, TC>(a, &e, r, false);
        EXPECT(a.gyro == nullptr);   // the bearing form
        e.in_b_bound = nullptr;
        ukfb::bind_sensor_inputs<TS, TC>(a, &e, r, false);
        EXPECT(a.gyro == nullptr);
    }
}

int main() {
    check_precision_choice();
    check_model_dispatch();
    check_binders<double, double>();   // fp64
    check_binders<float, double>();    // fp32 arrays, wide arithmetic
    check_binders<float, float>();     // fp32
    return finish();
}
