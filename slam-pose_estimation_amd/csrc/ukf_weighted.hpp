// ukf_weighted.hpp -- the sensor-frame update with GIVEN association weights (include/ukf_batch_jpda.h): the
// probabilistic data association update (ukf_pda.hpp) whose weights are read, not computed -- the joint marginals of
// ukf_jpda_kernel, or anything else a caller normalised.
//
// Layout, LDS map (sensor_map), device functions (assoc_measure, pda_score, row_apply_delta) and the statements up to the
// candidate loop are the PDA kernel's, by inclusion.  What differs:
//  * no exponent and no running maximum: the loop accumulates the UNNORMALISED sums s = sum w, sum w y, sum w nu, sum w y y^T
//    with w_k = weight_k where the candidate is scored with a finite d^2 and the weight is finite and > 0, else 0.  The gate
//    cfg.gate_chi2 plays no part;
//  * after the loop one division: c = max(1, s), beta_0 = 1 - s / c, y-bar, nu-bar, P_y, and M = (s / c) I - P_y;
//  * the second, store-only pass writes weight_used = w_k / c and needs no score again: the loop left one bit per candidate
//    (d^2 finite) in a register.  As in the PDA kernel it also rewrites the streamed scores of a filter whose Sigma~ failed,
//    and a wave-uniform branch skips it when nobody wants it.
// A filter that fails, uses no weight, is inactive or uninitialised rides along: every select is per row, no row's bits depend
// on its wave-mates.  commit = 0: the kernel gets NULL for the state's output pointers.
#pragma once

#include "ukf_pda.hpp"

namespace ukfb {

template <class T, class TS> struct WeightedArgs {
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
    const TS* point;             // [n][3] or null: point_u
    T mount_u[7], point_u[3];
    const TS* gyro;              // OrientationState: the latched rotation rate [n][3]
    T mean_tol;
    int mean_max_it;
    const TS* weight;            // [candidates][n]
    TS* z_pred;                  // [n][3] or null
    TS* S;                       // [n][9] or null
    TS* innov;                   // [candidates][n][3] or null
    TS* maha;                    // [candidates][n] or null
    TS* loglik;                  // [candidates][n] or null
    TS* weight_used;             // [candidates][n] or null
    TS* beta0;                   // [n] or null
    TS* innov_comb;              // [n][3] or null
    int32_t* n_used;             // [n] or null
    uint32_t* status;            // [n] or null
};

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_weighted_kernel(const WeightedArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2;
    constexpr SensorMap LY = sensor_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(2 * D * ZS <= LY.MUF - LY.TAB && SENSOR_INPUT_SCALARS <= LY.DUM - LY.INP, "W, Y and the input record fit their regions");
    static_assert(UKFB_ASSOCIATE_MAX_CANDIDATES <= 32, "one bit per candidate");
    extern __shared__ __attribute__((aligned(16))) unsigned char weighted_smem[];

    const RowCoords<M> rc(a.n, threadIdx.x);
    const int l = rc.l, lr = rc.lr, ls = rc.ls;
    const bool fvalid = rc.fvalid;
    const int64_t f = rc.f;
    T* const base = row_slice<T, LY.PF>(weighted_smem, rc.g);
    T *const FAC = base + LY.FAC, *const RSP = base + LY.RSP, *const TAB = base + LY.TAB, *const WT = base + LY.WT;
    T *const YM = base + LY.YM, *const MUF = base + LY.MUF, *const PKF = base + LY.PKF, *const INP = base + LY.INP;
    T* const DUMP = base + LY.DUM;

    // ---- the row's filter, model and records: Q, mount and the point; the candidates are streamed below
    const bool live = fvalid && a.initialised[f] != 0;
    const int mid = a.model ? a.model[f] : a.model_uniform;
    const bool mvalid = sensor_model_ok(M::MODEL, int64_t(mid));
    const int id = mvalid ? mid : (M::MODEL == 0 ? int(UKFB_SENSOR_POSE_POSITION) : int(UKFB_SENSOR_ORIENT_VELOCITY));   // no valid id: the row rides along
    const int m = sensor_meas_dim(id);
    row_stage_state<T, PK>(MUF, PKF, a.mu, a.cov, f * S, f * PK, l, ls);
    bool bad;
    {
        bool b = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i = l + 16 * p;
            const bool rec = i < SENSOR_INPUT_SCALARS;
            const bool is_z = i < SENSOR_INPUT_Q, is_q = !is_z && i < SENSOR_INPUT_MOUNT, is_m = rec && !is_z && !is_q && i < SENSOR_INPUT_POINT;
            const bool is_p = rec && i >= SENSOR_INPUT_POINT;
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
            const bool used = (is_q || is_m || is_p) && sensor_input_used(int64_t(id), i);   // z: judged per candidate
            b = b || (used && !m_finite(v));
            INP[i] = used ? v : ((i == SENSOR_INPUT_MOUNT + 6) ? T(1) : T(0));
        }
        bad = row_any(b);
    }
    wsync();
    const bool do_0 = live && mvalid && !bad;   // before the candidates are seen

    UKFB_MARK("w_sigma");
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

    UKFB_MARK("w_measure");
    // ================================================================= 2 - 4. z-bar, S = Ls Ls^T, Y = C Ls^-T: once
    AssocHyp<T> hy;
    assoc_measure<T, M>(xp, xm, id, m, hin, need_fwd, need_point, need_sens, do_0 && ok1, a.mean_tol, a.mean_max_it, FAC, INP, WT, DUMP, l, lr, hy);

    UKFB_MARK("w_candidates");
    // ================================================================= 5. per candidate: the scores and the unnormalised sums
    const T nanv = m_nan<T>();
    const T m_ln2pi = T(m) * T(1.8378770664093454835606594728112);
    const bool can_score = do_0 && ok1 && hy.ok2;
    T sw = T(0);
    T sy[3] = {T(0), T(0), T(0)}, snu[3] = {T(0), T(0), T(0)}, syy[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    uint32_t finite_bits = 0u;   // bit k: candidate k is scored and its d^2 is finite
    int n_used = 0;
    bool any_present = false;
#pragma nounroll
    for (int k = 0; k < a.candidates; ++k) {
        const int64_t slot = int64_t(k) * a.n + f;
        const PdaScore<T> sc = pda_score<T, TS>(a.z, slot, m, hy);
        const T wk = T(a.weight[slot]);
        const bool scored = can_score && sc.present;
        const bool finite = scored && m_finite(sc.d2);
        const bool used = finite && m_finite(wk) && wk > T(0);
        any_present = any_present || sc.present;
        finite_bits |= finite ? (1u << k) : 0u;
        n_used += used ? 1 : 0;
        {
            const T w = used ? wk : T(0);
            sw += w;
            T yk[3], nuk[3];   // (selects: y of a candidate that is not used never meets the sums)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                yk[c] = used ? sc.y[c] : T(0);
                nuk[c] = used ? sc.nu[c] : T(0);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const T wy = w * yk[c];
                sy[c] += wy;
                snu[c] = fma(w, nuk[c], snu[c]);
#pragma unroll
                for (int d = 0; d <= c; ++d) syy[c * (c + 1) / 2 + d] = fma(wy, yk[d], syy[c * (c + 1) / 2 + d]);
            }
        }
        const T nu_l = assoc_pick3(sc.nu[0], sc.nu[1], sc.nu[2], l);
        sfence();
        if (fvalid) {
            if (l < 3 && a.innov) a.innov[slot * 3 + l] = TS((l < m) ? (scored ? nu_l : nanv) : T(0));
            if (l == 0) {
                if (a.maha) a.maha[slot] = TS(scored ? sc.d2 : nanv);
                if (a.loglik) a.loglik[slot] = TS(scored ? T(-0.5) * (sc.d2 + hy.lndet + m_ln2pi) : nanv);
            }
        }
    }
    const bool conv = hy.conv;
    const bool any_scored = can_score && any_present;
    const bool any_finite = finite_bits != 0u;
    const bool do_u = do_0 && any_present;
    const bool accept = n_used > 0;

    UKFB_MARK("w_combine");
    // ================================================================= 6. c = max(1, s), beta_0, y-bar, nu-bar, M = (s / c) I - P_y
    const T inv = T(1) / (sw > T(1) ? sw : T(1));
    const T share = sw * inv;            // s / c = 1 - beta_0
    const T beta0 = T(1) - share;
    T yb[3], nub[3], m6[6];
    {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            yb[c] = sy[c] * inv;
            nub[c] = snu[c] * inv;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d <= c; ++d) {
                const T py = fma(-yb[c], yb[d], syy[c * (c + 1) / 2 + d] * inv);
                m6[c * (c + 1) / 2 + d] = ((c == d) ? share : T(0)) - py;
            }
    }
    T cr[3], wr[3];   // the lane's rows of Y and of W = Y M; no weight used: both zero
#pragma unroll
    for (int c = 0; c < 3; ++c) cr[c] = accept ? hy.cr[c] : T(0);
    wr[0] = fma(cr[2], m6[3], fma(cr[1], m6[1], cr[0] * m6[0]));
    wr[1] = fma(cr[2], m6[4], fma(cr[1], m6[2], cr[0] * m6[1]));
    wr[2] = fma(cr[2], m6[5], fma(cr[1], m6[4], cr[0] * m6[3]));
    wsync();   // W of assoc_measure is dead
    {
        T* const dst = (l < D) ? (YM + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = cr[c];
    }
    wsync();
    UKFB_MARK("w_cov");
    // ================================================================= 7. Sigma~ = Sigma - (Y M) Y^T: row lr, and delta = Y y-bar
    T sg[D], del[D];
    {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T* yc = YM + c * ZS;   // the rows other lanes wrote
            sg[c] = fma(-wr[2], yc[2], fma(-wr[1], yc[1], fma(-wr[0], yc[0], PKF[hi * (hi + 1) / 2 + lo])));
        }
        const T dl = fma(cr[2], yb[2], fma(cr[1], yb[1], cr[0] * yb[0]));
        static_for<0, D>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            del[c] = row_bcast<c>(dl);
        });
    }
    wsync();   // Y and the factor of Sigma are dead
    UKFB_MARK("w_commit");
    // ================================================================= 8. commit: applyDelta(mu, Sigma~, delta)
    T mnew[S];
    const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mnew);
    const bool okc = ok1 && any_scored && (!accept || ok3);
    const bool good = do_u && okc && accept;
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!mvalid ? ST_INACTIVE : ((bad || !any_present) ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && ok1 && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && any_finite && !accept) ? ST_REJECTED_GATE : 0u;

    UKFB_MARK("w_store");
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
    const T zbar_l = assoc_pick3(T(hy.z0[0] + TH(hy.ref[0])), T(hy.z0[1] + TH(hy.ref[1])), T(hy.z0[2] + TH(hy.ref[2])), l);
    const T s9_l = assoc_s9(hy.s6, m, l);
    const T nub_l = assoc_pick3(nub[0], nub[1], nub[2], l);
    sfence();
    if (fvalid) {
        if (l < 3 && a.z_pred) a.z_pred[f * 3 + l] = TS(scored_f ? ((l < m) ? zbar_l : T(0)) : nanv);
        if (a.S && l < 9) a.S[f * 9 + l] = TS(scored_f ? s9_l : nanv);
        if (l < 3 && a.innov_comb) a.innov_comb[f * 3 + l] = TS((l < m) ? (scored_f ? nub_l : nanv) : T(0));
        if (l == 0) {
            if (a.beta0) a.beta0[f] = TS(scored_f ? beta0 : nanv);
            if (a.n_used) a.n_used[f] = scored_f ? n_used : 0;
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
    // ---- the second pass: weight_used = w_k / c from the bits the loop left; a filter whose Sigma~ failed: the scores streamed
    // above become NaN (store-only; no row reads them)
    const bool undo = fvalid && do_u && any_scored && ok1 && accept && !ok3;
    if (a.weight_used != nullptr || wave_any(undo)) {
#pragma nounroll
        for (int k = 0; k < a.candidates; ++k) {
            const int64_t slot = int64_t(k) * a.n + f;
            const T wk = T(a.weight[slot]);
            const bool finite = scored_f && ((finite_bits >> k) & 1u) != 0u;
            const bool used = finite && m_finite(wk) && wk > T(0);
            sfence();
            if (fvalid && l == 0 && a.weight_used) a.weight_used[slot] = TS(finite ? (used ? wk * inv : T(0)) : nanv);
            if (undo) {
                if (l < m && a.innov) a.innov[slot * 3 + l] = TS(nanv);
                if (l == 0) {
                    if (a.maha) a.maha[slot] = TS(nanv);
                    if (a.loglik) a.loglik[slot] = TS(nanv);
                }
            }
        }
    }
}

}  // namespace ukfb
