// ukf_delayed.hpp -- late samples: the delayed-measurement update through the state history.  The smoother's backward chain
// runs from the engine's present state down to the step a late sample was taken at, the operator M (the product of the chain's
// gains and transports) is carried along it, ukfom's measurement half is made on the smoothed past state and the correction is
// retrodicted to the present and committed there.  Definitions: include/ukf_batch.h ("late samples"), DESIGN.md 4.20.
//
// Layout: the smoother's (ukf_smooth.hpp) -- one filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup, the
// chain resident in LDS between the steps, the opaque lane move in the step loop -- and its device functions in its order.
//  * M takes another D x LS region of LDS per filter; lane l < D owns row l.  One step's M <- A G J M is: the three rotation
//    COLUMNS of the lane's row of G times Jr^-1 inside the lane (G J), one row x matrix product with broadcast reads of M from
//    LDS (the row of G J goes through the dead factor region, as the smoother's (G M) row does), and the three rotation ROWS
//    times Jr over the rotation's lanes (DPP broadcasts).  J and A are block identities, so the two "congruences" are 3 x 3 work.
//  * Jr(phi) = I - a [phi]x + b [phi]x^2 in closed form from cos_sinc_fast: a = (1 - cos t) / t^2 = sinc(t / 2)^2 / 2 has no
//    cancellation at any angle in the half-angle form, b = (t - sin t) / t^3 = (1 - sinc(t / 2) cos(t / 2)) / t^2 above
//    t^2 = 1/4 and its series below (the split of bank_jrinv_coeff).  The alternative, a 3 x 3 inverse of the Jr^-1 the chain
//    already forms, costs a determinant, a division and nine cofactors and inherits Jr^-1's rounding; the closed form is one
//    more cos_sinc_fast and six multiply-adds.
//  * per-filter lags: the step loop runs to the wavefront's largest lag; a row whose lag is reached (or whose chain broke, or
//    that has no sample) freezes chain and M and rides along -- per-row selects, no divergence in what wave-mates compute.
//  * after the loop every row runs the measurement half once on its chain record: the sigma points of (mu^s, Sigma^s), h = the
//    model's M::measure (ids 0 ... 9, per-row selects between the vector models and the SO(3) one), the iterated mean, S in
//    registers on every lane (six row all-reductions), C_z row = sum_j L[l][j] W_j, Y_s = C_z Ls^-T.
//  * retrodiction, all row-local: lane l forms row l of N = Sigma_n M^T (broadcast reads of M), solves it against the factor of
//    Sigma^s (the smoother's two triangular solves per row: P = N (Sigma^s)^-1) and takes Y_n row l = sum_j P[l][j] Y_s[j].
//    For lag 0 M = I, N = Sigma^s and P = I to rounding.
//  * commit: Sigma~_n = Sigma_n - Y_n Y_n^T, applyDelta(mu_n, Sigma~_n, Y_n y) as the sensor-measurement kernel.
//  * commit = 0: the kernel gets NULL for the engine's state pointers -- it has nothing through which it could store there.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.  Plain fp32 holds the
//    1e-4 gate without any fp64 piece (tests/test_delayed_reference.py: the all-float32 evaluation is 2e-6 from the float64 one).
// LDS per filter: delayed_map (ukf_host.hpp) -- the smoother's slice and the rows of M behind it.
// The chain (steps 1-2) is ukf_delayed_chain.inc.hpp, included in the kernel body: the relative update (ukf_relative.hpp) runs it too.
// Steps 3d-5 are ukf_delayed_retro.inc.hpp, included likewise: the late sensor-frame samples (ukf_delayed_sensor.hpp) run them too.
#pragma once

#include "ukf_row.hpp"
#include "ukf_bank.hpp"          // bank_jrinv_coeff
#include "ukf_smooth.hpp"
#include "ukf_sensor_meas.hpp"   // sensor_solve3

namespace ukfb {

template <class T, class TS> struct DelayedArgs {
    int64_t n;                   // filters
    const TS* mu;                // [n][S]   the engine's state: the chain's start and what the commit corrects
    const TS* cov;               // [n][PK]
    TS* eng_mu;                  // the same arrays for commit = 1, null for commit = 0
    TS* eng_cov;
    uint32_t* engine_status;     // [n]; null for commit = 0
    const TS* mu_hist;           // [slots][n][S]
    const TS* cov_hist;          // [slots][n][PK]
    int slots, top_slot, back;   // ring size, slot of step n (never read), backward steps of the window (steps - 1)
    const uint8_t* initialised;  // [n]
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
    int lag_uniform;
    const int32_t* lag;          // [n] or null
    int model_uniform;
    const int32_t* model;        // [n] or null
    const TS* z;                 // [n][3]
    const TS* Q;                 // [n][9], or [9] when q_uniform
    int q_uniform;
    T gate_chi2;                 // < 0: accept
    TS* z_pred;                  // [n][4] or null
    TS* S;                       // [n][9] or null
    TS* innov;                   // [n][3] or null
    TS* maha;                    // [n] or null
    TS* loglik;                  // [n] or null
    uint32_t* status;            // [n] or null
    TS* mu_out;                  // [n][S] or null
    TS* cov_out;                 // [n][PK] or null
    double dt[SMOOTH_MAX_BACK];  // dt[k]: time step of the prediction redone by backward step k (step n - 1 - k -> n - k)
};

// (a, b) of Jr(phi) = I - a [phi]x + b [phi]x^2 as functions of t = theta^2 (see the head of the file)
template <class T> UKFB_DEV void delayed_jr_coeffs(T t, T& a, T& b) {
    T ch, sh;
    cos_sinc_fast(T(0.25) * t, ch, sh);   // cos(theta / 2), sinc(theta / 2)
    a = T(0.5) * sh * sh;
    T s = T(1. / 1307674368000.);
    s = fma(s, t, T(-1. / 6227020800.));
    s = fma(s, t, T(1. / 39916800.));
    s = fma(s, t, T(-1. / 362880.));
    s = fma(s, t, T(1. / 5040.));
    s = fma(s, t, T(-1. / 120.));
    s = fma(s, t, T(1. / 6.));
    const bool big = !(t <= T(0.25));
    const T closed = fma(-sh, ch, T(1)) * fast_rcp(big ? t : T(1));
    b = big ? closed : s;
}

// rows li = 0 ... 2 of I + ca [phi]x + cb [phi]x^2 (Jr: ca = -a, cb = b; Jr^-1: ca = 1/2, cb = bank_jrinv_coeff), row-major
template <class T> UKFB_DEV void delayed_rot_matrix(const T (&p)[3], T t, T ca, T cb, T (&B)[9]) {
    const T p0 = p[0], p1 = p[1], p2 = p[2];
    B[0] = fma(cb, p0 * p0 - t, T(1)); B[1] = fma(cb, p0 * p1, -ca * p2); B[2] = fma(cb, p0 * p2, ca * p1);
    B[3] = fma(cb, p1 * p0, ca * p2); B[4] = fma(cb, p1 * p1 - t, T(1)); B[5] = fma(cb, p1 * p2, -ca * p0);
    B[6] = fma(cb, p2 * p0, -ca * p1); B[7] = fma(cb, p2 * p1, ca * p0); B[8] = fma(cb, p2 * p2 - t, T(1));
}

// What a row derives from its lane index (the smoother's SmoothRow over the wider slice, and the rows of M)
template <class T, class M, class TS> struct DelayedRow {
    static constexpr DelayedMap LY = delayed_map(M::S, M::D);   // the LDS slice (ukf_host.hpp): the smoother's, widened
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(3 * M::D * LY.ZS <= LY.CSM - LY.TAB, "W, Y_s and Y_n fit the delta table");
    int l, lr, ls;
    bool fvalid, live;
    int64_t f;
    T *FAC, *RSP, *TAB, *GM, *MM, *CSM, *CSP, *MUF, *PKF, *ROT, *DUMP, *SMR, *MUP, *MOP;
    const TS *Rn, *Racc;
    UKFB_DEV DelayedRow(const DelayedArgs<T, TS>& a, unsigned char* smem, int lane) {
        const int g = lane >> 4;
        l = lane & 15;
        lr = (l < M::D) ? l : (M::D - 1);
        ls = (l < M::S) ? l : (M::S - 1);
        const int64_t wg0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * ROW_FILTERS_PER_GROUP;
        const int64_t n_here = a.n - wg0;
        const int n_wg = int(n_here < ROW_FILTERS_PER_GROUP ? n_here : int64_t(ROW_FILTERS_PER_GROUP));
        fvalid = g < n_wg;
        f = wg0 + (fvalid ? g : (n_wg - 1));   // rows beyond the batch repeat its last filter and store nothing
        live = fvalid && a.initialised[f] != 0;
        T* const base = reinterpret_cast<T*>(smem) + g * LY.PF;
        FAC = base + LY.FAC; RSP = base + LY.RSP; TAB = base + LY.TAB; GM = base + LY.GM; MM = base + LY.MM;
        CSM = base + LY.CSM; CSP = base + LY.CSP; MUF = base + LY.MUF; PKF = base + LY.PKF; ROT = base + LY.ROT;
        DUMP = base + LY.DUM; SMR = base + LY.SMR; MUP = base + LY.MUP; MOP = base + LY.MOP;
        Rn = a.Rn + f * a.Rn_stride;
        Racc = a.Racc + f * a.Rn_stride;
    }
};

// What a row's sample asks for: model, lag and whether the row takes part at all (the same from every lane of the row)
template <class T, class M, class TS> struct DelayedSample {
    int midc, m, reach;
    bool so3, mvalid, inactive, old, bad, do_u;
    T zin[3];
    UKFB_DEV DelayedSample(const DelayedArgs<T, TS>& a, int64_t f, bool live) {
        const int mid = a.model ? a.model[f] : a.model_uniform;
        const int lag = a.lag ? a.lag[f] : a.lag_uniform;
        mvalid = M::meas_valid(mid);
        midc = mvalid ? mid : (M::MODEL == 0 ? 0 : 9);
        m = M::meas_dim(midc);
        so3 = M::meas_is_so3(midc);
        inactive = lag < 0 || !mvalid;
        old = !inactive && lag > a.back;
#pragma unroll
        for (int c = 0; c < 3; ++c) zin[c] = T(a.z[f * 3 + c]);
        bad = !(m_finite(zin[0]) && (m < 2 || m_finite(zin[1])) && (m < 3 || m_finite(zin[2])));
        do_u = live && !inactive && !old && !bad;
        reach = do_u ? lag : 0;
    }
};

// The row's coordinates above, the factorisations and the two commits below are the statements of RowCoords, row_factorise and
// row_apply_delta (ukf_row.hpp) in place: called from here they change this kernel's instruction mix (branch layout, lane
// reads) and the fp32 instantiation left the spread of the parent's own runs (profiles/row_toolkit_rates.txt), so it keeps them
// as it was tuned.
template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_delayed_kernel(const DelayedArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr DelayedMap LY = delayed_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q, RT = MT<M>::RT;
    extern __shared__ __attribute__((aligned(16))) unsigned char delayed_smem[];
    uint32_t st = ST_OK;
    bool chain_ok = true;
    using ChainSample = DelayedSample<T, M, TS>;
#include "ukf_delayed_chain.inc.hpp"

    // ======================================================================= after the loop: the sample meets the smoothed past state
    const DelayedRow<T, M, TS> row(a, delayed_smem, threadIdx.x);
    const auto& [l, lr, ls, fvalid, live, f, FAC, RSP, TAB, GM, MM, CSM, CSP, MUF, PKF, ROT, DUMP, SMR, MUP, MOP, Rn, Racc] = row;
    const DelayedSample<T, M, TS> smp(a, f, live);
    const int midc = smp.midc, m = smp.m;
    const bool so3 = smp.so3, do_u = smp.do_u;
    T* const WT = TAB + (LY.WT - LY.TAB);
    T* const YM = TAB + (LY.YM - LY.TAB);
    T* const YN = TAB + (LY.YN - LY.TAB);
    // the engine's present state into the (dead) filtered-record region
    MUF[l] = T(a.mu[f * S + ls]);
    for (int i = l; i < PK; i += 16) PKF[i] = T(a.cov[f * PK + i]);
    wsync();
    UKFB_MARK("d_sigma");
    // ================================================================= 3a. sigma points of (mu^s, Sigma^s) and Z = h(X)
    bool ok1;
    T zp[4], zm[4], z0[4];
    {
        T mu_r[S], xp[S], xm[S];
#pragma unroll
        for (int s = 0; s < S; ++s) mu_r[s] = CSM[s];
        T arow[D];
        load_row<T, D>(CSP, l, arow);
        const T rs = chol16<T, D, LS>(arow, FAC, l, ok1);
        wsync();
        row_scale_factor<T, D, LS>(FAC, RSP, l, rs);   // the scaled columns stay: C_z and the retrodiction's solves read them
        T col[D];
        load_column<T, D, LS>(FAC, l, T(1), col);
        sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: the centre twice
        sfence();
        M::measure(xp, midc, zp);
        M::measure(xm, midc, zm);
#pragma unroll
        for (int c = 0; c < 4; ++c) z0[c] = row_bcast<D>(zp[c]);
    }
    sfence();
    UKFB_MARK("d_mean");
    // ================================================================= 3b. z-bar: ukfom's iterated mean (R^m, or SO(3) for model 3)
    const bool any_so3 = wave_any(so3);
    const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
    T ref[4] = {z0[0], z0[1], z0[2], z0[3]};
    bool conv = true;
    {
        bool active = do_u && chain_ok && ok1;
        int it = 0;
        while (wave_any(active)) {
            T rp[3] = {T(0), T(0), T(0)}, rm[3] = {T(0), T(0), T(0)};
            if (any_so3) {
                rot_minus(zp, ref, rp);
                rot_minus(zm, ref, rm);
            }
            T dp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = fma(wm, so3 ? rm[c] : (zm[c] - ref[c]), wp * (so3 ? rp[c] : (zp[c] - ref[c])));
            row_allreduce_n<T, 3>(dp);
            T m2 = T(0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dp[c] *= T(1) / T(N);
                m2 = fma(dp[c], dp[c], m2);
            }
            T nq[4] = {T(0), T(0), T(0), T(1)};
            if (any_so3) {
                T ex[4];
                so3_exp_fast(dp, T(1), ex);
                quat_mul(ref, ex, nq);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) ref[c] = active ? (so3 ? nq[c] : (ref[c] + dp[c])) : ref[c];
            ref[3] = (active && so3) ? nq[3] : ref[3];
            const bool more = m2 > a.mean_tol * a.mean_tol;
            const bool capped = more && (it + 1 >= a.mean_max_it);
            it += (active && more) ? 1 : 0;
            conv = conv && !(active && capped);
            active = active && more && !capped;
        }
    }
    UKFB_MARK("d_stats");
    // ================================================================= 3c. S = 1/2 sum dz dz^T + Q (identity beyond m), nu, W to LDS
    T s6[6], nu[3];
    {
        T dpv[3], dmv[3], nv[3];
        {
            T rp[3] = {T(0), T(0), T(0)}, rm[3] = {T(0), T(0), T(0)}, rn[3] = {T(0), T(0), T(0)};
            if (any_so3) {
                rot_minus(zp, ref, rp);
                rot_minus(zm, ref, rm);
                T zq[4];
                so3_exp_fast(smp.zin, T(1), zq);   // RotationType(SO3::exp(z)), as ukfb_update_dev
                rot_minus(zq, ref, rn);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dpv[c] = so3 ? rp[c] : (zp[c] - ref[c]);
                dmv[c] = so3 ? rm[c] : (zm[c] - ref[c]);
                nv[c] = so3 ? rn[c] : ((c < m) ? (smp.zin[c] - ref[c]) : T(0));
            }
        }
        T u[3], w[3];
        const T fu = (l == D) ? T(0.70710678118654752440) : T(1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u[c] = wp * (fu * (T(0.5) * (dpv[c] + dmv[c])));   // the centre's row: delta_0 / sqrt 2; lanes beyond it: nothing
            w[c] = wm * (T(0.5) * (dpv[c] - dmv[c]));
            nu[c] = nv[c];
        }
        T* const dst = (l < D) ? (WT + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = w[c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) s6[r * (r + 1) / 2 + c] = fma(u[r], u[c], w[r] * w[c]);
        row_allreduce_n<T, 6>(s6);
        const TS* qp = a.Q + (a.q_uniform ? int64_t(0) : f * 9);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const T q = T(qp[3 * r + c]);
                s6[r * (r + 1) / 2 + c] = (r < m) ? (s6[r * (r + 1) / 2 + c] + q) : ((r == c) ? T(1) : T(0));   // (c <= r < m)
            }
    }
    wsync();
#include "ukf_delayed_retro.inc.hpp"

    UKFB_MARK("d_store");
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
            T v = ref[0];
#pragma unroll
            for (int c = 1; c < 4; ++c) v = (l == c) ? ref[c] : v;
            a.z_pred[f * 4 + l] = TS(scored ? ((so3 || l < m) ? v : T(0)) : nanv);
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
