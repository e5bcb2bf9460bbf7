// ukf_forecast.hpp -- forecast on the device: a chain of predictions from a start record into rings of the history's format,
// READ-ONLY on the engine: every pointer the kernel gets into the engine's state is a pointer to const.  Definitions:
// include/ukf_batch.h ("forecast"), DESIGN.md 4.18.  The forward counterpart of ukf_smooth.hpp.
//
// Layout: the tuned one (ukf_kernel16.hpp) -- one filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup.
//  * chain residency: the start record is loaded once; the chain (mean, packed covariance) stays in LDS in the compute type
//    between the steps of a launch; per step only the inputs come in from HBM and only one record leaves, narrowed TS(...) once
//    at its store.  The chain itself is never narrowed.
//  * the step is the smoother's phase 1 with the row toolkit's device functions (ukf_row.hpp) in its order (row_factorise, load_column,
//    sigma_pair, process_fast, the iterated mean, row_publish_deltas, row_table_row, process_noise_entry16): lane l < D owns the
//    sigma pair of factor column l, lane D the centre, and afterwards row l of Sigma^-, whose lower triangle goes to the chain.
//    No cross-covariance, no solve, no transport, no applyDelta.
//  * the time step of a row: dt[c] by value, or (ts form) from the step's stamp and the row's SHADOW last measurement time,
//    which starts at the engine's (read on the device) and advances as predictionStepFromSampleTime advances it.
//  * a filter that fails, is gated or is uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates (the mean iteration runs while any row is active; a converged row keeps its reference).
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// LDS per filter: forecast_map (ukf_host.hpp) -- the factor region (Sigma's factor, then the rows of Sigma^-), the
// delta table, the chain record, the rotation matrix, a sink.
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

template <class T, class TS> struct ForecastArgs {
    int64_t n;                   // filters
    const TS* start_mu;          // [n][S]   the start record: the engine's state or the caller's
    const TS* start_cov;         // [n][PK]
    TS* mu_out;                  // [slots][n][S]
    TS* cov_out;                 // [slots][n][PK] or null
    int slots, first_slot, steps;   // ring size, slot of step 0, steps of this launch (<= FORECAST_MAX_STEPS)
    int use_ts;                  // the time steps come from ts_us and the shadow last measurement time
    const uint8_t* initialised;  // [n]
    const int64_t* last_ts;      // [n]: where the shadow time starts (ts form)
    const TS* Rn;                // process noise, D * D row-major; per filter if Rn_stride != 0
    int64_t Rn_stride;
    const TS* Racc;              // Pose: acceleration-branch noise (same stride)
    const TS* in_a;              // [n][3], or [slots][n][3] when in_ring & 1
    const TS* in_b;              // [n][3], or [slots][n][3] when in_ring & 2
    int in_ring;
    T ninv_tau_g, ninv_tau_a, earth[3];
    T mean_tol;
    int mean_max_it;
    double min_dt, max_dt;
    uint32_t* status;            // [n] or null
    double dt[FORECAST_MAX_STEPS];      // dt[c]: time step of the prediction that produces step c
    int64_t ts_us[FORECAST_MAX_STEPS];  // ts_us[c]: its stamp (ts form)
};

// What a row derives from its lane index; its LDS slice is forecast_map's (ukf_host.hpp).  Public members in this order: the step
// loop binds them by name
template <class T, class M, class TS> struct ForecastRow {
    static constexpr ForecastMap LY = forecast_map(M::S, M::D);
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    int l, lr, ls;       // lane of the row; clamped to a row of the matrices / an entry of the mean
    bool fvalid, live;   // the row has a filter of the batch; ... that is initialised: the row stores
    int64_t f;           // rows beyond the batch repeat its last filter and store nothing
    T *FAC, *RSP, *TAB, *CSM, *CSP, *ROT, *DUMP;
    const TS *Rn, *Racc;
    UKFB_DEV ForecastRow(const ForecastArgs<T, TS>& a, unsigned char* smem, int lane) {
        const RowCoords<M> rc(a.n, lane);
        l = rc.l; lr = rc.lr; ls = rc.ls; fvalid = rc.fvalid; f = rc.f;
        live = fvalid && a.initialised[f] != 0;
        T* const base = row_slice<T, LY.PF>(smem, rc.g);
        FAC = base + LY.FAC; RSP = base + LY.RSP; TAB = base + LY.TAB; CSM = base + LY.CSM; CSP = base + LY.CSP;
        ROT = base + LY.ROT; DUMP = base + LY.DUM;
        Rn = a.Rn + f * a.Rn_stride;
        Racc = a.Racc + f * a.Rn_stride;
    }
};

// (the second bound: wavefronts per SIMD the register allocator must leave room for)
template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_forecast_kernel(const ForecastArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr ForecastMap LY = forecast_map(S, D);
    constexpr int LS = LY.LS;
    extern __shared__ __attribute__((aligned(16))) unsigned char forecast_smem[];
    uint32_t st = ST_OK;
    int slot = a.first_slot;
    int64_t last = 0;   // the row's shadow last measurement time (ts form); the engine's is never written
    {
        // ---- the chain's start record
        const ForecastRow<T, M, TS> r(a, forecast_smem, threadIdx.x);
        st = (r.fvalid && !r.live) ? ST_UNINITIALISED : ST_OK;
        r.CSM[r.l] = T(a.start_mu[r.f * S + r.ls]);
        for (int i = r.l; i < PK; i += 16) r.CSP[i] = T(a.start_cov[r.f * PK + i]);
        if (a.use_ts) last = a.last_ts[r.f];
        wsync();
    }
#pragma nounroll
    for (int k = 0; k < a.steps; ++k) {
        // As in ukf_smooth.hpp: everything derived from the lane index is invariant over the steps and would be hoisted out of the
        // loop and held across every step -- more registers than the kernel has.  The lane index passes through an opaque move in
        // every step and its derivatives are formed again.
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        const ForecastRow<T, M, TS> row(a, forecast_smem, lane);
        const auto& [l, lr, ls, fvalid, live, f, FAC, RSP, TAB, CSM, CSP, ROT, DUMP, Rn, Racc] = row;
        const int64_t rec = int64_t(slot) * a.n + f;
        // ---- the inputs of the prediction that produces this step
        ProcIn<T> pin;
        {
            const TS* pa = a.in_a + (((a.in_ring & 1) ? int64_t(slot) * a.n : int64_t(0)) + f) * 3;
            const TS* pb = a.in_b + (((a.in_ring & 2) ? int64_t(slot) * a.n : int64_t(0)) + f) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pin.a[c] = T(pa[c]);
                pin.w[c] = T(pb[c]);
            }
        }
        // ---- the time step and its gate, ukfb_predict's own; ts form: predictionStepFromSampleTime on the shadow time
        double dt = a.dt[k];
        bool first = false;
        if (a.use_ts) {
            const int64_t ts = a.ts_us[k];
            first = last == 0;
            dt = first ? 0.0 : double(ts - last) / 1000000.0;
            last = (first || dt > a.min_dt) ? ts : last;
        }
        const bool neg = dt < 0.0, small = dt <= a.min_dt, large = dt > a.max_dt;
        const uint32_t code = first ? ST_SKIPPED_FIRST_TS : (neg ? ST_ERR_NEG_DT : (small ? ST_SKIPPED_SMALL_DT : (large ? ST_ERR_DT_TOO_LARGE : 0u)));
        st |= live ? code : 0u;
        const bool dof = live && code == 0u;   // a gated step makes no prediction: the chain passes through
        pin.dt = T(dt);
        pin.ninv_tau_g = a.ninv_tau_g;
        pin.ninv_tau_a = a.ninv_tau_a;
#pragma unroll
        for (int c = 0; c < 3; ++c) pin.earth[c] = a.earth[c];
        pin.use_acc = m_finite(pin.a[0]) && m_finite(pin.a[1]) && m_finite(pin.a[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) pin.adt[c] = pin.use_acc ? pin.dt * pin.a[c] : T(0);
        wsync();

        if (wave_any(dof)) {
            UKFB_MARK("f_predict");
            T mu_r[S], xp[S], xm[S], ref[S];
#pragma unroll
            for (int s = 0; s < S; ++s) mu_r[s] = CSM[s];
            {
                T q[4], rot[9];
                M::orientation(mu_r, q);
                quat_to_matrix(q, rot);
                T* dst = (l == 0) ? ROT : DUMP;
#pragma unroll
                for (int c = 0; c < 9; ++c) dst[c] = rot[c];
            }
            bool ok;
            {
                ok = row_factorise<T, D, LS>(CSP, FAC, RSP, l);
                T col[D];
                load_column<T, D, LS>(FAC, l, T(1), col);
                sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: the centre twice (their column is zero)
            }
            sfence();
            UKFB_MARK("f_process");
            process_fast((M*)nullptr, xp, pin);
            sfence();
            process_fast((M*)nullptr, xm, pin);
            sfence();
#pragma unroll
            for (int s = 0; s < S; ++s) ref[s] = row_bcast<D>(xp[s]);   // the propagated centre starts the mean
            UKFB_MARK("f_mean");
            bool conv = true;
            {
                const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
                bool active = dof && ok;
                int it = 0;
                while (wave_any(active)) {
                    T dp[D], dm[D];
                    row_boxminus<T, M>(xp, ref, dp);
                    row_boxminus<T, M>(xm, ref, dm);
#pragma unroll
                    for (int c = 0; c < D; ++c) dp[c] = fma(wm, dm[c], wp * dp[c]);
                    row_allreduce_n<T, D>(dp);
                    T m2 = T(0);
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        dp[c] *= T(1) / T(N);
                        m2 = fma(dp[c], dp[c], m2);
                    }
                    T nr[S];
                    row_boxplus<T, M>(ref, dp, nr);
#pragma unroll
                    for (int s = 0; s < S; ++s) ref[s] = active ? nr[s] : ref[s];
                    const bool more = m2 > a.mean_tol * a.mean_tol;
                    const bool capped = more && (it + 1 >= a.mean_max_it);
                    it += (active && more) ? 1 : 0;
                    conv = conv && !(active && capped);
                    active = active && more && !capped;
                }
            }
            UKFB_MARK("f_deltas");
            row_publish_deltas<T, M, LS>(TAB, DUMP, l, xp, xm, ref);
            wsync();   // (the factor is dead: every lane has its column)
            // Sigma^- = 1/2 sum delta delta^T + R: row lr, parked in the factor region while the noise is added entry by entry
            {
                T sm[D];
                row_table_row<T, D, LS>(TAB, N, lr, sm);
                sfence();
#pragma unroll
                for (int c = 0; c < D; ++c) FAC[lr * LS + c] = sm[c];   // (lanes >= D: row D - 1's own bits again)
            }
            sfence();
#pragma nounroll
            for (int c = 0; c < D; ++c) {
                const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;   // the noise's lower triangle, as the forward kernel reads it
                const T nz = (c < 6) ? process_noise_entry16<T, M, TS>(Rn, Racc, ROT, pin, hi, lo)
                                     : plain_noise_entry16<T, M, TS>(Rn, Racc, pin, hi, lo);
                FAC[lr * LS + c] += nz;
            }
            sfence();
            UKFB_MARK("f_chain");
            const bool good = dof && ok;
            st |= (dof && !ok) ? ST_ERR_CHOLESKY : 0u;
            st |= (good && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
            // the chain moves on: the predicted record; a failed or gated row keeps every bit of the record before it
            {
                T v = ref[0];
#pragma unroll
                for (int s = 1; s < S; ++s) v = (ls == s) ? ref[s] : v;
                T* dst = (good && l < S) ? (CSM + l) : DUMP;
                *dst = v;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const bool own = good && l < D && c <= l;
                    T* dc = own ? (CSP + lr * (lr + 1) / 2 + c) : DUMP;
                    *dc = FAC[lr * LS + c];
                }
            }
            wsync();
        }
        UKFB_MARK("f_store");
        // ---- the record of this step leaves
        if (live) {
            if (l < S) a.mu_out[rec * S + l] = TS(CSM[l]);
            if (a.cov_out)
                for (int i = l; i < PK; i += 16) a.cov_out[rec * PK + i] = TS(CSP[i]);
        }
        slot = (slot + 1 == a.slots) ? 0 : (slot + 1);
        wsync();
    }
    {
        const ForecastRow<T, M, TS> r(a, forecast_smem, threadIdx.x);
        if (r.fvalid && a.status && r.l == 0) a.status[r.f] = st;
    }
}

}  // namespace ukfb
