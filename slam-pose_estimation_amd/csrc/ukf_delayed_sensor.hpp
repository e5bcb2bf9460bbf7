// ukf_delayed_sensor.hpp -- late sensor-frame samples: the delayed update (ukf_delayed.hpp) with the sensor-frame measurements'
// h (ukf_sensor_meas.hpp).  A lever-arm fix, range or landmark sighting taken `lag` steps ago is evaluated on the sigma points of
// the smoothed past state of its own step and its correction is retrodicted to the present.  Definitions:
// include/ukf_batch_delayed_sensor.h, DESIGN.md 4.29.
//
// Layout: the delayed kernel's -- one filter per 16-lane row, four per wavefront, one wavefront per workgroup, its chain
// (ukf_delayed_chain.inc.hpp) and its LDS slice, not one scalar wider (delayed_sensor_map).
//  * the chain asks the row's sample for its reach in every step (ChainSample): DelayedSensorSample judges the 25 input scalars
//    lane-owned -- lane i loads entries i and i + 16 and looks at its own, one row vote -- and keeps nothing but flags.
//  * after the loop the same 25 scalars are staged ONCE into the parked rows of Sigma^- (dead since the chain ended), an entry the
//    row's model does not read replaced by its neutral value, as the sensor kernel stages its 22: a NaN there never meets
//    arithmetic.  Entries 22 ... 24 are the rotation rate at the time of the sample (ORIENT_VELOCITY): the caller's array, else
//    the rotation-rate ring's entry of step s when the ring is bound and lag >= 1, else the engine's latch.
//  * the sigma pair of (mu^s, Sigma^s), sensor_h on both points in fp64 in every mode with wave-uniform need_fwd / need_point /
//    need_sens, and the differences Z_i - Z_0, z - Z_0 in fp64: the head of ukf_sensor_meas.hpp says why.  From there the
//    measurement side works in coordinates whose origin is Z_0 (the sensor kernel's steps 3-4), the measurement space is R^3
//    whatever the model (m = 1 embedded with zero deltas and identity rows of S).  There is no SO(3) measurement here.
//  * C_z, the 3 x 3 factor in registers, the retrodiction, Sigma~_n, the commit and the call's status are the delayed kernel's
//    steps 3d-5, one statement of each: ukf_delayed_retro.inc.hpp, included in both kernel bodies as the chain is.  The delayed
//    kernel's mean and statistics (3b, 3c) work in absolute coordinates with per-row SO(3) selects, this kernel's in coordinates
//    relative to Z_0, and z_pred is formed differently, so those steps and the stores stand in each kernel.
//  * TS (storage) / T (compute) as in ukf_delayed.hpp.
#pragma once

#include "ukf_delayed.hpp"

namespace ukfb {

// The delayed update's arguments (z [n][3], Q [n][9] or [9], z_pred [n][4]; model / model_uniform hold UKFB_SENSOR_* ids) and
// what the sensor-frame h reads beside them
template <class T, class TS> struct DelayedSensorArgs : DelayedArgs<T, TS> {
    const TS* mount;             // [n][7] or null: mount_u
    const TS* point;             // [n][3] or null: point_u
    T mount_u[7], point_u[3];
    const TS* rate;              // [n][3] the rotation rate at the time of the sample, or null
    const TS* gyro;              // OrientationState: the latched rotation rate [n][3]; null for Pose
};

static_assert(DELAYED_SENSOR_INPUT_SCALARS <= DELAYED_SENSOR_INPUT_REGION && DELAYED_SENSOR_INPUT_REGION == 32, "lane l stages entries l and l + 16");

// Entry i of the row's input record (SENSOR_INPUT_*, then the rate) as the arguments hold it; an index beyond the record loads a
// safe address and is never used.  slot_s: the ring slot of the sample's step (for the rate ring).
template <class T, class M, class TS>
UKFB_DEV T delayed_sensor_entry(const DelayedSensorArgs<T, TS>& a, int64_t f, int i, bool ring_rate, int slot_s) {
    const bool is_z = i < SENSOR_INPUT_Q, is_q = !is_z && i < SENSOR_INPUT_MOUNT, is_m = !is_z && !is_q && i < SENSOR_INPUT_POINT;
    const bool is_p = i >= SENSOR_INPUT_POINT && i < SENSOR_INPUT_SCALARS;
    const bool is_w = M::MODEL == 1 && i >= DELAYED_SENSOR_INPUT_RATE && i < DELAYED_SENSOR_INPUT_SCALARS;
    const bool from_arg = (is_m && !a.mount) || (is_p && !a.point);
    const TS* src = a.z + f * 3;   // (a safe address for the lanes that load nothing)
    src = is_z ? (a.z + f * 3 + i) : src;
    src = is_q ? (a.Q + (a.q_uniform ? int64_t(0) : f * 9) + (i - SENSOR_INPUT_Q)) : src;
    src = (is_m && a.mount) ? (a.mount + f * 7 + (i - SENSOR_INPUT_MOUNT)) : src;
    src = (is_p && a.point) ? (a.point + f * 3 + (i - SENSOR_INPUT_POINT)) : src;
    if constexpr (M::MODEL == 1) {
        const TS* w = a.rate ? (a.rate + f * 3) : (ring_rate ? (a.in_b + (int64_t(slot_s) * a.n + f) * 3) : (a.gyro + f * 3));
        src = is_w ? (w + (i - DELAYED_SENSOR_INPUT_RATE)) : src;
    }
    T v = T(*src);
    T av = T(0);
#pragma unroll
    for (int k = 0; k < 7; ++k) av = (i == SENSOR_INPUT_MOUNT + k) ? a.mount_u[k] : av;
#pragma unroll
    for (int k = 0; k < 3; ++k) av = (i == SENSOR_INPUT_POINT + k) ? a.point_u[k] : av;
    return from_arg ? av : v;
}

// What a row's sample asks for: model, lag, where its rate comes from and whether the row takes part at all (the same from
// every lane of the row; every lane of the wavefront constructs it -- the judgement of the inputs is a row vote)
template <class T, class M, class TS> struct DelayedSensorSample {
    int id, m, reach, slot_s;
    bool mvalid, inactive, old, bad, do_u, ring_rate;
    UKFB_DEV DelayedSensorSample(const DelayedSensorArgs<T, TS>& a, int64_t f, bool live) {
        const int mid = a.model ? a.model[f] : a.model_uniform;
        const int lag = a.lag ? a.lag[f] : a.lag_uniform;
        mvalid = sensor_model_ok(M::MODEL, int64_t(mid));
        id = mvalid ? mid : (M::MODEL == 0 ? int(UKFB_SENSOR_POSE_POSITION) : int(UKFB_SENSOR_ORIENT_VELOCITY));   // no valid id: the row rides along
        m = sensor_meas_dim(id);
        inactive = lag < 0 || !mvalid;
        old = !inactive && lag > a.back;
        const int lagc = (lag >= 1 && lag <= a.back) ? lag : 0;   // (back <= slots - 1)
        ring_rate = (a.in_ring & 2) != 0 && lagc >= 1;
        slot_s = (a.top_slot - lagc + a.slots) % a.slots;
        const int l = int(threadIdx.x) & 15;
        bool b = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i = l + 16 * p;
            const T v = delayed_sensor_entry<T, M, TS>(a, f, i, ring_rate, slot_s);
            b = b || (delayed_sensor_input_used(int64_t(id), i) && !m_finite(v));
        }
        bad = row_any(b);
        do_u = live && !inactive && !old && !bad;
        reach = do_u ? lag : 0;
    }
};

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_delayed_sensor_kernel(const DelayedSensorArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr DelayedSensorMap LY = delayed_sensor_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q, RT = MT<M>::RT;
    // the input record lives in the parked rows of Sigma^-: inside them, and they overlap nothing that is live after the chain
    static_assert(LY.INP == LY.SMR && DELAYED_SENSOR_INPUT_REGION <= D * LS, "the input record fits the parked rows of Sigma^-");
    static_assert(LY.SMR >= LY.DUM + 16 && LY.SMR + D * LS <= LY.MUP && LY.MUP + 16 <= LY.MOP, "the parked rows lie between the sink and mu^-, below M");
    static_assert(LY.SMR >= LY.PKF + PK && LY.SMR >= LY.CSP + PK && LY.SMR >= LY.TAB + N * LS && LY.SMR >= LY.RSP + 16,
                  "factor, table and both records end below the input record");
    static_assert(LY.PF == delayed_map(S, D).PF, "the delayed update's slice, not one scalar wider");
    extern __shared__ __attribute__((aligned(16))) unsigned char delayed_smem[];
    uint32_t st = ST_OK;
    bool chain_ok = true;
    using ChainSample = DelayedSensorSample<T, M, TS>;
#include "ukf_delayed_chain.inc.hpp"

    // ======================================================================= after the loop: the sample meets the smoothed past state
    const DelayedRow<T, M, TS> row(a, delayed_smem, threadIdx.x);
    const auto& [l, lr, ls, fvalid, live, f, FAC, RSP, TAB, GM, MM, CSM, CSP, MUF, PKF, ROT, DUMP, SMR, MUP, MOP, Rn, Racc] = row;
    const DelayedSensorSample<T, M, TS> smp(a, f, live);
    const int id = smp.id, m = smp.m;
    const bool do_u = smp.do_u;
    T* const WT = TAB + (LY.WT - LY.TAB);
    T* const YM = TAB + (LY.YM - LY.TAB);
    T* const YN = TAB + (LY.YN - LY.TAB);
    T* const INP = SMR + (LY.INP - LY.SMR);
    // the engine's present state into the (dead) filtered-record region
    MUF[l] = T(a.mu[f * S + ls]);
    for (int i = l; i < PK; i += 16) PKF[i] = T(a.cov[f * PK + i]);
    // ---- the input record, once: the entry, or its neutral value where the row's model does not read it
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int i = l + 16 * p;
        const T v = delayed_sensor_entry<T, M, TS>(a, f, i, smp.ring_rate, smp.slot_s);
        INP[i] = delayed_sensor_input_used(int64_t(id), i) ? v : ((i == SENSOR_INPUT_MOUNT + 6) ? T(1) : T(0));
    }
    wsync();
    UKFB_MARK("ds_sigma");
    // ================================================================= 3a. sigma points of (mu^s, Sigma^s) and Z = h(X), relative to Z_0
    // h, and the differences of its values to the centre's, are evaluated in fp64 in every mode (ukf_sensor_meas.hpp)
    using TH = double;
    bool ok1;
    T zp[3], zm[3], zin[3], ref[3] = {T(0), T(0), T(0)};
    TH z0[3];
    {
        T mu_r[S], xp[S], xm[S];
#pragma unroll
        for (int s = 0; s < S; ++s) mu_r[s] = CSM[s];
        SensorIn<TH> hin;
        {
            const TH q0 = TH(mu_r[Q]), q1 = TH(mu_r[Q + 1]), q2 = TH(mu_r[Q + 2]), q3 = TH(mu_r[Q + 3]);
            hin.rnq = fast_rcp(fma(q0, q0, fma(q1, q1, fma(q2, q2, q3 * q3))));
        }
        T arow[D];
        load_row<T, D>(CSP, l, arow);
        const T rs = chol16<T, D, LS>(arow, FAC, l, ok1);
        wsync();
        row_scale_factor<T, D, LS>(FAC, RSP, l, rs);   // the scaled columns stay: C_z and the retrodiction's solves read them
        T col[D];
        load_column<T, D, LS>(FAC, l, T(1), col);
        sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: the centre twice
        sfence();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            hin.r[c] = TH(INP[SENSOR_INPUT_MOUNT + c]);
            hin.b[c] = TH(INP[SENSOR_INPUT_POINT + c]);
            hin.gy[c] = TH(INP[DELAYED_SENSOR_INPUT_RATE + c]);
        }
        {
            const TH qs[4] = {TH(INP[SENSOR_INPUT_MOUNT + 3]), TH(INP[SENSOR_INPUT_MOUNT + 4]), TH(INP[SENSOR_INPUT_MOUNT + 5]),
                              TH(INP[SENSOR_INPUT_MOUNT + 6])};
            const TH rn = fast_rcp(fma(qs[0], qs[0], fma(qs[1], qs[1], fma(qs[2], qs[2], qs[3] * qs[3]))));
            hin.qsi[0] = -qs[0] * rn; hin.qsi[1] = -qs[1] * rn; hin.qsi[2] = -qs[2] * rn; hin.qsi[3] = qs[3] * rn;
        }
        const bool need_sens = wave_any(sensor_reads_rotation(int64_t(id)));
        const bool need_point = wave_any(id == UKFB_SENSOR_POSE_POINT);
        const bool need_fwd = wave_any(id == UKFB_SENSOR_POSE_POSITION || id == UKFB_SENSOR_POSE_RANGE || id == UKFB_SENSOR_POSE_NAV_VELOCITY);
        using MH = typename M::template rebind<TH>;
        TH xh[S], zph[3], zmh[3];
#pragma unroll
        for (int s = 0; s < S; ++s) xh[s] = TH(xp[s]);
        sensor_h((MH*)nullptr, xh, id, hin, need_fwd, need_point, need_sens, zph);
        sfence();
#pragma unroll
        for (int s = 0; s < S; ++s) xh[s] = TH(xm[s]);
        sensor_h((MH*)nullptr, xh, id, hin, need_fwd, need_point, need_sens, zmh);
        sfence();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            z0[c] = row_bcast<D>(zph[c]);   // Z_0 starts the mean
            zp[c] = T(zph[c] - z0[c]);
            zm[c] = T(zmh[c] - z0[c]);
            zin[c] = T(TH(INP[SENSOR_INPUT_Z + c]) - z0[c]);   // z - Z_0 (beyond m: 0 - 0)
        }
    }
    sfence();
    UKFB_MARK("ds_mean");
    // ================================================================= 3b. z-bar - Z_0: ukfom's iterated mean on R^3
    bool conv = true;
    const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
    {
        bool active = do_u && chain_ok && ok1;
        int it = 0;
        while (wave_any(active)) {
            T dp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = fma(wm, zm[c] - ref[c], wp * (zp[c] - ref[c]));
            row_allreduce_n<T, 3>(dp);
            T m2 = T(0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dp[c] *= T(1) / T(N);
                m2 = fma(dp[c], dp[c], m2);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) ref[c] = active ? (ref[c] + dp[c]) : ref[c];
            const bool more = m2 > a.mean_tol * a.mean_tol;
            const bool capped = more && (it + 1 >= a.mean_max_it);
            it += (active && more) ? 1 : 0;
            conv = conv && !(active && capped);
            active = active && more && !capped;
        }
    }
    UKFB_MARK("ds_stats");
    // ================================================================= 3c. S = 1/2 sum dz dz^T + Q (identity beyond m), nu, W to LDS
    T s6[6], nu[3], zbar[3];
    {
        T u[3], w[3];
        const T fu = (l == D) ? T(0.70710678118654752440) : T(1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T dp = zp[c] - ref[c], dm = zm[c] - ref[c];
            u[c] = wp * (fu * (T(0.5) * (dp + dm)));      // the centre's row: delta_0 / sqrt 2; lanes beyond it: nothing
            w[c] = wm * (T(0.5) * (dp - dm));
        }
        T* const dst = (l < D) ? (WT + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = w[c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) s6[r * (r + 1) / 2 + c] = fma(u[r], u[c], w[r] * w[c]);
        row_allreduce_n<T, 6>(s6);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const T q = INP[SENSOR_INPUT_Q + 3 * r + c];
                s6[r * (r + 1) / 2 + c] = (r < m) ? (s6[r * (r + 1) / 2 + c] + q) : ((r == c) ? T(1) : T(0));   // (c <= r < m)
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            nu[c] = zin[c] - ref[c];
            zbar[c] = T(z0[c] + TH(ref[c]));
        }
    }
    wsync();
#include "ukf_delayed_retro.inc.hpp"

    UKFB_MARK("ds_store");
    // ---- the new state through LDS (the records are dead), then whole rows of the packed arrays
    // (in place in every kernel: as a shared function the block spilled to scratch, which the build gate refuses)
    {
        T v = mnew[0];
#pragma unroll
        for (int s = 1; s < S; ++s) v = (ls == s) ? mnew[s] : v;
        T* const dm = (l < S) ? (MUF + l) : DUMP;
        *dm = v;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const bool own = l < D && c <= l;
            T* const dc = own ? (PKF + lr * (lr + 1) / 2 + c) : DUMP;
            *dc = sg[c];
        }
    }
    wsync();
    const T nanv = m_nan<T>();
    if (good && a.eng_mu) {
        if (l < S) a.eng_mu[f * S + l] = TS(MUF[l]);
        for (int i = l; i < PK; i += 16) a.eng_cov[f * PK + i] = TS(PKF[i]);
    }
    if (fvalid) {
        if (a.mu_out && l < S) a.mu_out[f * S + l] = TS(good ? MUF[l] : nanv);
        if (a.cov_out)
            for (int i = l; i < PK; i += 16) a.cov_out[f * PK + i] = TS(good ? PKF[i] : nanv);
        const bool scored = do_u && okc;
        if (a.z_pred && l < 4) {
            T v = zbar[0];
#pragma unroll
            for (int c = 1; c < 3; ++c) v = (l == c) ? zbar[c] : v;
            a.z_pred[f * 4 + l] = TS(scored ? ((l < m) ? v : T(0)) : nanv);
        }
        if (a.innov && l < 3) {
            T v = nu[0];
#pragma unroll
            for (int c = 1; c < 3; ++c) v = (l == c) ? nu[c] : v;
            a.innov[f * 3 + l] = TS(scored ? ((l < m) ? v : T(0)) : nanv);
        }
        if (a.S && l < 9) {
            T v = T(0);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int r = k / 3, c = k % 3, hi = r > c ? r : c, lo = r > c ? c : r;
                v = (l == k) ? ((hi < m) ? s6[hi * (hi + 1) / 2 + lo] : T(0)) : v;
            }
            a.S[f * 9 + l] = TS(scored ? v : nanv);
        }
        if (l == 0) {
            const T m_ln2pi = T(m) * T(1.8378770664093454835606594728112);
            if (a.maha) a.maha[f] = TS(scored ? d2 : nanv);
            if (a.loglik) a.loglik[f] = TS(scored ? T(-0.5) * (d2 + lndet + m_ln2pi) : nanv);
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
}

}  // namespace ukfb
