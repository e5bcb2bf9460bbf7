// ukf_predict_sampled.hpp -- user-defined process models: ukfom's predict(f, R) finished from the propagated sigma points
// XX_i = f(X_i) the caller evaluated on the export of ukf_sampled.hpp, and the caller's R; a read-only mode.
// Definitions: include/ukf_batch.h ("user-defined process models"), DESIGN.md 4.22.
//
// Layout: the tuned one (ukf_kernel16.hpp) -- one filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup.
// The kernel IS the back half of ukf_forecast_kernel (ukf_forecast.hpp): everything that kernel does before process_fast
// (rotation matrix, factorisation, sigma spread, the model) is replaced by a staged load, its model-specific noise by R:
//  * the record in global memory is the export's, filter-major ([n][2 D + 1][S]).  The row copies its filter's (2 D + 1) S
//    contiguous scalars into LDS with 16-lane coalesced loads (and judges them: ERR_NONFINITE_MEAS), then lane l < D takes rows
//    1 + 2 l and 2 + 2 l, lane D the centre, row 0: the xp / xm registers the forecast kernel's mean loop expects.  The staging
//    area aliases the delta table.
//  * the differences XX_i - XX_0 of every vector block are formed first, in fp64 in every mode (ukf_sampled.hpp, for its
//    reason), and the mean iteration and the deltas work on those differences: the prediction is invariant under a translation
//    of a vector block of all XX_i together.  XX_0 waits in the record's mean slot; the predicted vector blocks are XX_0 + the
//    mean difference, summed in fp64.  Quaternion blocks are used as given.
//  * from there the forecast kernel's statements in their order: the iterated mean with per-row `active`, row_publish_deltas,
//    row_table_row, the row of Sigma^- parked in LDS while the noise is added entry by entry.  The noise is R's lower-triangle
//    entry as it is stored; a uniform R is a stride of zero.
//  * nothing is factorised: the kernel reads neither Sigma nor the mean, and has no pointer to them but the output's.
//  * a filter that fails, is inactive or uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates (the mean iteration runs while any row is active; a converged row keeps its reference).
//  * commit = 0: the kernel gets NULL for the state's output pointers -- it has nothing through which it could store.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// LDS per filter: predict_sampled_map (ukf_host.hpp).
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

template <class T, class TS> struct PredictSampledArgs {
    int64_t n;                   // filters
    TS* mu_out;                  // the engine's [n][S] / [n][PK] for commit = 1, null for commit = 0
    TS* cov_out;
    uint32_t* engine_status;     // [n]; null for commit = 0
    const uint8_t* initialised;  // [n]
    const TS* XX;                // [n][2 D + 1][S]
    const TS* R;                 // D * D row-major; per filter if R_stride != 0
    int64_t R_stride;
    const uint8_t* active;       // [n] or null
    T mean_tol;
    int mean_max_it;
    TS* mu;                      // [n][S] or null
    TS* cov_packed;              // [n][PK] or null
    uint32_t* status;            // [n] or null
};

// (the second bound: wavefronts per SIMD the register allocator must leave room for)
template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_predict_sampled_kernel(const PredictSampledArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2, Q = MT<M>::Q;
    constexpr PredictSampledMap LY = predict_sampled_map(S, D);   // the LDS slice (ukf_host.hpp)
    constexpr int LS = LY.LS;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(N * S <= LY.CSM - LY.STG, "the staged samples fit the table they alias");
    extern __shared__ __attribute__((aligned(16))) unsigned char psm_smem[];

    // (RowCoords' statements in place: built on it, this kernel left the spread of the parent's own runs -- profiles/row_toolkit_rates.txt)
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int lr = (l < D) ? l : (D - 1), ls = (l < S) ? l : (S - 1);
    const int64_t wg0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * ROW_FILTERS_PER_GROUP;
    const int64_t n_here = a.n - wg0;
    const int n_wg = int(n_here < ROW_FILTERS_PER_GROUP ? n_here : int64_t(ROW_FILTERS_PER_GROUP));
    const bool fvalid = g < n_wg;
    const int64_t f = wg0 + (fvalid ? g : (n_wg - 1));   // rows beyond the batch repeat its last filter and store nothing
    T* const base = reinterpret_cast<T*>(psm_smem) + g * LY.PF;
    T *const SMR = base + LY.SMR, *const TAB = base + LY.TAB, *const STG = base + LY.STG, *const CSM = base + LY.CSM;
    T *const CSP = base + LY.CSP, *const DUMP = base + LY.DUM;
    const TS* const Rf = a.R + f * a.R_stride;

    // ---- the row's filter and its record: the samples to LDS, judged on the way; the lower triangle of R is judged where it
    // lies (the lane's row of the symmetric matrix: the entries the noise loop reads again below)
    const bool live = fvalid && a.initialised[f] != 0;
    const bool act = !a.active || a.active[f] != 0;
    bool bad;
    {
        bool b = false;
        const TS* const rec = a.XX + f * int64_t(N * S);
        constexpr int FULL = (N * S) / 16;
#pragma unroll
        for (int k = 0; k < FULL; ++k) {
            const T v = T(rec[l + 16 * k]);
            b = b || !m_finite(v);
            STG[l + 16 * k] = v;
        }
        if (l + 16 * FULL < N * S) {
            const T v = T(rec[l + 16 * FULL]);
            b = b || !m_finite(v);
            STG[l + 16 * FULL] = v;
        }
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            b = b || !m_finite(T(Rf[hi * D + lo]));
        }
        bad = row_any(b);
    }
    wsync();
    const bool dof = live && act && !bad;

    UKFB_MARK("p_take");
    // ---- the lane's pair.  Vector blocks relative to XX_0: the differences are formed in fp64 in every mode, before anything is
    // rounded to the compute type; quaternion blocks as they are.  Lanes >= D: the centre (twice)
    using TH = double;
    T xp[S], xm[S], ref[S];
    {
        const int ip = ((l < D) ? (1 + 2 * l) : 0) * S, im = ((l < D) ? (2 + 2 * l) : 0) * S;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const bool quat = s >= Q && s < Q + 4;
            const T vp = STG[ip + s], vm = STG[im + s], v0 = STG[s];
            xp[s] = quat ? vp : T(TH(vp) - TH(v0));
            xm[s] = quat ? vm : T(TH(vm) - TH(v0));
        }
        T* const d0 = (l < S) ? (CSM + l) : DUMP;
        *d0 = STG[ls];   // XX_0 waits in the record's mean slot
    }
    wsync();   // the staged samples are dead: the delta table may be written
#pragma unroll
    for (int s = 0; s < S; ++s) ref[s] = row_bcast<D>(xp[s]);   // the propagated centre starts the mean
    UKFB_MARK("p_mean");
    bool conv = true;
    {
        const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
        bool active = dof;
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
    UKFB_MARK("p_deltas");
    row_publish_deltas<T, M, LS>(TAB, DUMP, l, xp, xm, ref);
    wsync();
    // Sigma^- = 1/2 sum delta delta^T + R: row lr, parked while the noise is added entry by entry
    {
        T sm[D];
        row_table_row<T, D, LS>(TAB, N, lr, sm);
        sfence();
#pragma unroll
        for (int c = 0; c < D; ++c) SMR[lr * LS + c] = sm[c];   // (lanes >= D: row D - 1's own bits again)
    }
    sfence();
#pragma nounroll
    for (int c = 0; c < D; ++c) {
        const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;   // the noise's lower triangle
        SMR[lr * LS + c] += T(Rf[hi * D + lo]);
    }
    sfence();
    UKFB_MARK("p_record");
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!act ? ST_INACTIVE : (bad ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (dof && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    // ---- the predicted record through LDS: vector blocks XX_0 + the mean difference (summed in fp64), then whole rows
    // (the store block of the updates, but the mean's entry is formed on the way and the rows come from LDS)
    {
        T v = ref[0];
#pragma unroll
        for (int s = 1; s < S; ++s) v = (ls == s) ? ref[s] : v;
        const bool quat = ls >= Q && ls < Q + 4;
        T* const dm = (l < S) ? (CSM + l) : DUMP;
        const T x0 = CSM[ls];
        *dm = quat ? v : T(TH(x0) + TH(v));
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const bool own = l < D && c <= l;
            T* const dc = own ? (CSP + lr * (lr + 1) / 2 + c) : DUMP;
            *dc = SMR[lr * LS + c];
        }
    }
    wsync();
    UKFB_MARK("p_store");
    if (dof && a.mu_out) {
        if (l < S) a.mu_out[f * S + l] = TS(CSM[l]);
        for (int i = l; i < PK; i += 16) a.cov_out[f * PK + i] = TS(CSP[i]);
    }
    if (fvalid) {
        const T nanv = m_nan<T>();
        if (l < S && a.mu) a.mu[f * S + l] = TS(dof ? CSM[l] : nanv);
        if (a.cov_packed)
            for (int i = l; i < PK; i += 16) a.cov_packed[f * PK + i] = TS(dof ? CSP[i] : nanv);
        if (l == 0) {
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
}

}  // namespace ukfb
