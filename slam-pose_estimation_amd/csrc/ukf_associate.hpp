// ukf_associate.hpp -- sensor-frame association: the sensor-frame measurement update (ukf_sensor_meas.hpp) scored against K
// candidate samples per filter in one launch, the nearest candidate inside the gate chosen by ukfb_innovation_dev's rule and,
// with commit = 1, the update finished with it.  Definitions: include/ukf_batch.h ("sensor-frame association"), DESIGN.md 4.26.
//
// Layout, LDS map (sensor_map) and device functions are the sensor kernel's: one filter per 16-lane DPP row, lane l < D owns
// the sigma pair of factor column l, lane D the centre; h is sensor_h itself, S, its factor and the solves are the same
// statements in the same order.  What differs:
//  * step 1 (chol(Sigma), the sigma pair in registers) runs once and stays resident over the candidate loop;
//  * HYP = false (shared-h mode: K detections against one hypothesis): Z_i, z-bar, S, C, Ls, Y run once before the loop, and a
//    candidate costs a load of z, nu = z - z-bar, y = Ls^-1 nu, two scalars and its stores;
//  * HYP = true (per-hypothesis mode: candidate k pairs z[k] with the point b[k]): those steps run per candidate on the resident
//    sigma pair; W goes through LDS per candidate, the lane's row of Y and y of the best candidate so far stay in registers, so
//    that the commit needs no second pass over h.  The mode is the call's: a row whose model does not read b takes the same
//    path with its neutral point and gets K equal hypotheses;
//  * candidates are streamed: z[k] (and b[k]) are loaded with row-uniform addresses, innov / maha / loglik (and z_pred / S per
//    hypothesis) are stored as they are formed; only a running (best d^2, index, count) is kept;
//  * an absent candidate (a non-finite entry among its first m of z, or of the b[k] its model reads) is replaced by neutral
//    values before anything computes with it, scores NaN and is never best;
//  * the verdict on Sigma~ is known after the loop only: a filter whose accepted update fails there (ERR_CHOLESKY: all float
//    outputs NaN) rewrites its streamed scores in a second, store-only pass that a wave-uniform branch skips otherwise.
// A filter that fails, is gated, inactive or uninitialised rides along: every select is per row, no row's bits depend on its
// wave-mates.  commit = 0: the kernel gets NULL for the state's output pointers.
#pragma once

#include "ukf_sensor_meas.hpp"

namespace ukfb {

template <class T, class TS> struct AssociateArgs {
    int64_t n;                   // filters: the stride of a candidate's slot
    const TS* mu;                // [n][S]
    const TS* cov;               // [n][PK]
    TS* mu_out;                  // the same arrays for commit = 1, null for commit = 0
    TS* cov_out;
    uint32_t* engine_status;     // [n]; null for commit = 0
    const uint8_t* initialised;  // [n]
    int model_uniform;
    const int32_t* model;        // [n] or null
    int candidates;              // 1 ... 32
    const TS* z;                 // [candidates][n][3]
    const TS* Q;                 // [n][9], or [9] when q_uniform
    int q_uniform;
    const TS* mount;             // [n][7] or null: mount_u
    const TS* point;             // HYP: [candidates][n][3]; else [n][3] or null: point_u
    T mount_u[7], point_u[3];
    const TS* gyro;              // OrientationState: the latched rotation rate [n][3]
    T mean_tol;
    int mean_max_it;
    T gate_chi2;                 // < 0: every finite candidate is inside
    TS* z_pred;                  // [H][n][3] or null; H = candidates (HYP) or 1
    TS* S;                       // [H][n][9] or null
    TS* innov;                   // [candidates][n][3] or null
    TS* maha;                    // [candidates][n] or null
    TS* loglik;                  // [candidates][n] or null
    int32_t* best;               // [n] or null
    int32_t* n_gated;            // [n] or null
    uint32_t* status;            // [n] or null
};

// One hypothesis: what steps 2 - 4 of the sensor update leave behind.  ref = z-bar - Z_0, z0 = Z_0 (fp64 in every mode), s6 =
// the lower triangle of S, (l10, l20, l21, rs) = its factor, cr = the lane's row of Y = C Ls^-T.
template <class T> struct AssocHyp {
    T ref[3], s6[6], cr[3], rs[3];
    double z0[3];
    T l10, l20, l21, lndet;
    bool ok2, conv;
};

// Steps 2 - 4 of ukf_sensor_meas_kernel for the point hin.b, on the lane's sigma pair (xp, xm): the statements of that kernel in
// their order.  `active`: the row iterates its mean.  W goes to WT; the caller synchronises before WT is written again.
template <class T, class M>
UKFB_DEV void assoc_measure(const T (&xp)[M::S], const T (&xm)[M::S], int id, int m, const SensorIn<double>& hin, bool need_fwd, bool need_point,
                            bool need_sens, bool active, T mean_tol, int mean_max_it, const T* FAC, const T* INP, T* WT, T* DUMP, int l,
                            int lr, AssocHyp<T>& hy) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1;
    constexpr SensorMap LY = sensor_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS;
    using TH = double;
    // ---- 2. Z = h(X) on the lane's pair, relative to Z_0
    T zp[3], zm[3];
    {
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
            hy.z0[c] = row_bcast<D>(zph[c]);   // Z_0 starts the mean
            zp[c] = T(zph[c] - hy.z0[c]);
            zm[c] = T(zmh[c] - hy.z0[c]);
            hy.ref[c] = T(0);
        }
    }
    sfence();
    // ---- 3. z-bar - Z_0: ukfom's iterated mean on R^3
    hy.conv = true;
    const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
    {
        int it = 0;
        while (wave_any(active)) {
            T dp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = fma(wm, zm[c] - hy.ref[c], wp * (zp[c] - hy.ref[c]));
            row_allreduce_n<T, 3>(dp);
            T m2 = T(0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dp[c] *= T(1) / T(N);
                m2 = fma(dp[c], dp[c], m2);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) hy.ref[c] = active ? (hy.ref[c] + dp[c]) : hy.ref[c];
            const bool more = m2 > mean_tol * mean_tol;
            const bool capped = more && (it + 1 >= mean_max_it);
            it += (active && more) ? 1 : 0;
            hy.conv = hy.conv && !(active && capped);
            active = active && more && !capped;
        }
    }
    // ---- 4. S = 1/2 sum dz dz^T + Q (identity beyond m), W to LDS
    {
        T u[3], w[3];
        const T fu = (l == D) ? T(0.70710678118654752440) : T(1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T dp = zp[c] - hy.ref[c], dm = zm[c] - hy.ref[c];
            u[c] = wp * (fu * (T(0.5) * (dp + dm)));
            w[c] = wm * (T(0.5) * (dp - dm));
        }
        T* const dst = (l < D) ? (WT + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = w[c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) hy.s6[r * (r + 1) / 2 + c] = fma(u[r], u[c], w[r] * w[c]);
        row_allreduce_n<T, 6>(hy.s6);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const T q = INP[SENSOR_INPUT_Q + 3 * r + c];
                hy.s6[r * (r + 1) / 2 + c] = (r < m) ? (hy.s6[r * (r + 1) / 2 + c] + q) : ((r == c) ? T(1) : T(0));
            }
    }
    wsync();
    // ---- C = sum_j (L col j) W_j^T: row lr
#pragma unroll
    for (int c = 0; c < 3; ++c) hy.cr[c] = T(0);
#pragma nounroll
    for (int j = 0; j < D; ++j) {
        const T lj = FAC[j * LS + lr];
        const T* w = WT + j * ZS;
#pragma unroll
        for (int c = 0; c < 3; ++c) hy.cr[c] = fma(lj, w[c], hy.cr[c]);
    }
    // ---- S = Ls Ls^T in registers; Y = C Ls^-T
    {
        const T d0 = hy.s6[0], i0 = fast_rcp(d0);
        const T t10 = hy.s6[1] * i0, t20 = hy.s6[3] * i0;
        const T d1 = fma(-t10, hy.s6[1], hy.s6[2]), a21 = fma(-t20, hy.s6[1], hy.s6[4]);
        const T i1 = fast_rcp(d1);
        const T d2p = fma(-(a21 * i1), a21, fma(-t20, hy.s6[3], hy.s6[5]));
        hy.ok2 = (d0 > T(0)) && (d1 > T(0)) && (d2p > T(0));   // (NaN fails every comparison)
        hy.lndet = m_log(d0) + m_log(d1) + m_log(d2p);          // a pivot beyond m is exactly 1
        hy.rs[0] = fast_rsqrt(d0);
        hy.rs[1] = fast_rsqrt(d1);
        hy.rs[2] = fast_rsqrt(d2p);
        hy.l10 = hy.s6[1] * hy.rs[0];
        hy.l20 = hy.s6[3] * hy.rs[0];
        hy.l21 = a21 * hy.rs[1];
        sensor_solve3(hy.cr, hy.l10, hy.l20, hy.l21, hy.rs);
    }
}

// lane k < 9 of a row: entry k of the row-major 3 x 3 whose leading m x m block is s6's matrix, the rest 0
template <class T> UKFB_DEV T assoc_s9(const T (&s6)[6], int m, int l) {
    T v = T(0);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int r = k / 3, c = k % 3, hi = r > c ? r : c, lo = r > c ? c : r;
        v = (l == k) ? ((hi < m) ? s6[hi * (hi + 1) / 2 + lo] : T(0)) : v;
    }
    return v;
}
// lane l of a row: entry l of (v0, v1, v2).  Called where nothing bounds l: under `l < 3` the compiler turns the selects into an
// indexed load of a private array, which is scratch
template <class T> UKFB_DEV T assoc_pick3(T v0, T v1, T v2, int l) { return (l == 2) ? v2 : ((l == 1) ? v1 : v0); }

template <class T, class M, class TS, bool HYP>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_associate_kernel(const AssociateArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2;
    constexpr SensorMap LY = sensor_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(2 * D * ZS <= LY.MUF - LY.TAB && SENSOR_INPUT_SCALARS <= LY.DUM - LY.INP, "W, Y and the input record fit their regions");
    extern __shared__ __attribute__((aligned(16))) unsigned char asc_smem[];

    const RowCoords<M> rc(a.n, threadIdx.x);
    const int l = rc.l, lr = rc.lr, ls = rc.ls;
    const bool fvalid = rc.fvalid;
    const int64_t f = rc.f;
    T* const base = row_slice<T, LY.PF>(asc_smem, rc.g);
    T *const FAC = base + LY.FAC, *const RSP = base + LY.RSP, *const TAB = base + LY.TAB, *const WT = base + LY.WT;
    T *const YM = base + LY.YM, *const MUF = base + LY.MUF, *const PKF = base + LY.PKF, *const INP = base + LY.INP;
    T* const DUMP = base + LY.DUM;

    // ---- the row's filter, model and records: Q, mount and (shared-h mode) the point; the candidates are streamed below
    const bool live = fvalid && a.initialised[f] != 0;
    const int mid = a.model ? a.model[f] : a.model_uniform;
    const bool mvalid = sensor_model_ok(M::MODEL, int64_t(mid));
    const int id = mvalid ? mid : (M::MODEL == 0 ? int(UKFB_SENSOR_POSE_POSITION) : int(UKFB_SENSOR_ORIENT_VELOCITY));   // no valid id: the row rides along
    const int m = sensor_meas_dim(id);
    const bool reads_b = sensor_reads_point(int64_t(id));
    row_stage_state<T, PK>(MUF, PKF, a.mu, a.cov, f * S, f * PK, l, ls);
    bool bad;
    {
        bool b = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i = l + 16 * p;
            const bool rec = i < SENSOR_INPUT_SCALARS;
            const bool is_z = i < SENSOR_INPUT_Q, is_q = !is_z && i < SENSOR_INPUT_MOUNT, is_m = rec && !is_z && !is_q && i < SENSOR_INPUT_POINT;
            const bool is_p = !HYP && rec && i >= SENSOR_INPUT_POINT;
            const bool from_arg = (is_m && !a.mount) || (is_p && !a.point);
            const TS* src = a.z + f * 3;   // (a safe address for the lanes that load nothing)
            src = is_q ? (a.Q + (a.q_uniform ? int64_t(0) : f * 9) + (i - SENSOR_INPUT_Q)) : src;
            src = (is_m && a.mount) ? (a.mount + f * 7 + (i - SENSOR_INPUT_MOUNT)) : src;
            src = (is_p && a.point) ? (a.point + f * 3 + (i - SENSOR_INPUT_POINT)) : src;
            T v = T(*src);
            T av = T(0);
#pragma unroll
            for (int k = 0; k < 7; ++k) av = (i == SENSOR_INPUT_MOUNT + k) ? a.mount_u[k] : av;
#pragma unroll
            for (int k = 0; k < 3; ++k) av = (i == SENSOR_INPUT_POINT + k) ? a.point_u[k] : av;
            v = from_arg ? av : v;
            const bool used = (is_q || is_m || is_p) && sensor_input_used(int64_t(id), i);   // z and the streamed points: judged per candidate
            b = b || (used && !m_finite(v));
            INP[i] = used ? v : ((i == SENSOR_INPUT_MOUNT + 6) ? T(1) : T(0));
        }
        bad = row_any(b);
    }
    wsync();
    const bool do_0 = live && mvalid && !bad;   // before the candidates are seen

    UKFB_MARK("a_sigma");
    // ================================================================= 1. sigma points of (mu, Sigma): once
    using TH = double;
    T xp[S], xm[S];
    bool ok1;
    SensorIn<TH> hin;
    {
        T mu_r[S];
#pragma unroll
        for (int s = 0; s < S; ++s) mu_r[s] = MUF[s];
        {
            const TH q0 = TH(mu_r[Q]), q1 = TH(mu_r[Q + 1]), q2 = TH(mu_r[Q + 2]), q3 = TH(mu_r[Q + 3]);
            hin.rnq = fast_rcp(fma(q0, q0, fma(q1, q1, fma(q2, q2, q3 * q3))));
        }
        ok1 = row_factorise<T, D, LS>(PKF, FAC, RSP, l);   // the scaled columns stay: C reads them
        T col[D];
        load_column<T, D, LS>(FAC, l, T(1), col);
        sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: the centre twice (their column is zero)
    }
    sfence();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        hin.r[c] = TH(INP[SENSOR_INPUT_MOUNT + c]);
        hin.b[c] = TH(INP[SENSOR_INPUT_POINT + c]);
        hin.gy[c] = TH(0);
    }
    if constexpr (M::MODEL == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) hin.gy[c] = TH(a.gyro[f * 3 + c]);
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

    AssocHyp<T> hy;
    if constexpr (!HYP) {
        UKFB_MARK("a_measure");
        assoc_measure<T, M>(xp, xm, id, m, hin, need_fwd, need_point, need_sens, do_0 && ok1, a.mean_tol, a.mean_max_it, FAC, INP, WT, DUMP, l, lr, hy);
    }

    UKFB_MARK("a_candidates");
    // ================================================================= 5. per candidate: nu, y = Ls^-1 nu, d^2, loglik; the best
    const T nanv = m_nan<T>();
    const T m_ln2pi = T(m) * T(1.8378770664093454835606594728112);
    const bool gate_on = !(a.gate_chi2 < T(0));
    T crb[3] = {T(0), T(0), T(0)}, yb[3] = {T(0), T(0), T(0)};   // the best candidate's row of Y and y; none: delta = 0
    T best_d2 = T(0);
    int best = -1, n_gated = 0;
    bool any_present = false, any_scored = false, any_finite = false, conv = true;
#pragma nounroll
    for (int k = 0; k < a.candidates; ++k) {
        const int64_t slot = int64_t(k) * a.n + f;
        T zk[3];
        bool present = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T v = T(a.z[slot * 3 + c]);
            present = present && (c >= m || m_finite(v));
            zk[c] = v;
        }
        if constexpr (HYP) {
            T bk[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                bk[c] = reads_b ? T(a.point[slot * 3 + c]) : T(0);   // (a model that does not read b never loads it)
                present = present && m_finite(bk[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) hin.b[c] = (reads_b && present) ? TH(bk[c]) : TH(0);
            wsync();   // the reads of W of the candidate before
            assoc_measure<T, M>(xp, xm, id, m, hin, need_fwd, need_point, need_sens, do_0 && ok1 && present, a.mean_tol, a.mean_max_it, FAC, INP, WT,
                                DUMP, l, lr, hy);
            conv = conv && (hy.conv || !present);
        }
        T nu[3], yn[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T zin = T(TH((c < m && present) ? zk[c] : T(0)) - hy.z0[c]);   // z - Z_0 (beyond m: 0 - 0)
            nu[c] = zin - hy.ref[c];
            yn[c] = nu[c];
        }
        sensor_solve3(yn, hy.l10, hy.l20, hy.l21, hy.rs);
        const T d2 = fma(yn[0], yn[0], fma(yn[1], yn[1], yn[2] * yn[2]));
        const bool scored = do_0 && ok1 && present && hy.ok2;
        const bool finite = scored && m_finite(d2);
        const bool inside = finite && (!gate_on || d2 <= a.gate_chi2);
        const bool better = inside && (best < 0 || d2 < best_d2);   // equal d^2: the lower index stays
        any_present = any_present || present;
        any_scored = any_scored || scored;
        any_finite = any_finite || finite;
        n_gated += inside ? 1 : 0;
        best = better ? k : best;
        best_d2 = better ? d2 : best_d2;
#pragma unroll
        for (int c = 0; c < 3; ++c) yb[c] = better ? yn[c] : yb[c];
        if constexpr (HYP) {
#pragma unroll
            for (int c = 0; c < 3; ++c) crb[c] = better ? hy.cr[c] : crb[c];
        }
        const T nu_l = assoc_pick3(nu[0], nu[1], nu[2], l);
        T zbar_l = T(0), s9_l = T(0);
        if constexpr (HYP) {
            zbar_l = assoc_pick3(T(hy.z0[0] + TH(hy.ref[0])), T(hy.z0[1] + TH(hy.ref[1])), T(hy.z0[2] + TH(hy.ref[2])), l);
            s9_l = assoc_s9(hy.s6, m, l);
        }
        sfence();
        if (fvalid) {
            if (l < 3) {
                if (a.innov) a.innov[slot * 3 + l] = TS((l < m) ? (scored ? nu_l : nanv) : T(0));
                if constexpr (HYP) {
                    if (a.z_pred) a.z_pred[slot * 3 + l] = TS(scored ? ((l < m) ? zbar_l : T(0)) : nanv);
                }
            }
            if constexpr (HYP) {
                if (a.S && l < 9) a.S[slot * 9 + l] = TS(scored ? s9_l : nanv);
            }
            if (l == 0) {
                if (a.maha) a.maha[slot] = TS(scored ? d2 : nanv);
                if (a.loglik) a.loglik[slot] = TS(scored ? T(-0.5) * (d2 + hy.lndet + m_ln2pi) : nanv);
            }
        }
    }
    if constexpr (!HYP) {
        conv = hy.conv;
#pragma unroll
        for (int c = 0; c < 3; ++c) crb[c] = hy.cr[c];
    }
    const bool do_u = do_0 && any_present;
    const bool accept = best >= 0;
    wsync();   // W is dead
    {
        T* const dst = (l < D) ? (YM + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = accept ? crb[c] : T(0);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) crb[c] = accept ? crb[c] : T(0);
    wsync();
    UKFB_MARK("a_cov");
    // ================================================================= 7. Sigma~ = Sigma - Y Y^T: row lr, and delta = Y y
    T sg[D], del[D];
    {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T* yc = YM + c * ZS;   // the rows other lanes wrote
            sg[c] = fma(-crb[2], yc[2], fma(-crb[1], yc[1], fma(-crb[0], yc[0], PKF[hi * (hi + 1) / 2 + lo])));
        }
        const T dl = fma(crb[2], yb[2], fma(crb[1], yb[1], crb[0] * yb[0]));
        static_for<0, D>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            del[c] = row_bcast<c>(dl);
        });
    }
    wsync();   // W, Y and the factor of Sigma are dead
    UKFB_MARK("a_commit");
    // ================================================================= 8. commit: applyDelta(mu, Sigma~, delta)
    T mnew[S];
    const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mnew);
    const bool okc = ok1 && any_scored && (!accept || ok3);
    const bool good = do_u && okc && accept;
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!mvalid ? ST_INACTIVE : ((bad || !any_present) ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && ok1 && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && any_finite && !accept) ? ST_REJECTED_GATE : 0u;

    UKFB_MARK("a_store");
    // ---- the new state through LDS (the records are dead), then whole rows of the packed arrays
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
    if (good && a.mu_out) {
        if (l < S) a.mu_out[f * S + l] = TS(MUF[l]);
        for (int i = l; i < PK; i += 16) a.cov_out[f * PK + i] = TS(PKF[i]);
    }
    const bool scored_f = do_u && okc;
    T zbar_l = T(0), s9_l = T(0);
    if constexpr (!HYP) {
        zbar_l = assoc_pick3(T(hy.z0[0] + TH(hy.ref[0])), T(hy.z0[1] + TH(hy.ref[1])), T(hy.z0[2] + TH(hy.ref[2])), l);
        s9_l = assoc_s9(hy.s6, m, l);
    }
    sfence();
    if (fvalid) {
        if constexpr (!HYP) {
            if (l < 3 && a.z_pred) a.z_pred[f * 3 + l] = TS(scored_f ? ((l < m) ? zbar_l : T(0)) : nanv);
            if (a.S && l < 9) a.S[f * 9 + l] = TS(scored_f ? s9_l : nanv);
        }
        if (l == 0) {
            if (a.best) a.best[f] = scored_f ? best : -1;
            if (a.n_gated) a.n_gated[f] = scored_f ? n_gated : 0;
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
    // ---- an accepted update whose Sigma~ failed: the scores streamed above become NaN (store-only; no row reads them)
    const bool undo = fvalid && do_u && any_scored && ok1 && accept && !ok3;
    if (wave_any(undo)) {
#pragma nounroll
        for (int k = 0; k < a.candidates; ++k) {
            const int64_t slot = int64_t(k) * a.n + f;
            if (undo) {
                if (l < m && a.innov) a.innov[slot * 3 + l] = TS(nanv);
                if constexpr (HYP) {
                    if (l < 3 && a.z_pred) a.z_pred[slot * 3 + l] = TS(nanv);
                    if (l < 9 && a.S) a.S[slot * 9 + l] = TS(nanv);
                }
                if (l == 0) {
                    if (a.maha) a.maha[slot] = TS(nanv);
                    if (a.loglik) a.loglik[slot] = TS(nanv);
                }
            }
        }
    }
}

}  // namespace ukfb
