// ukf_pda.hpp -- probabilistic data association: the shared-h sensor-frame association (ukf_associate.hpp, HYP = false) whose
// commit uses EVERY gated candidate at its posterior association weight instead of the nearest one at full weight.
// Definitions: include/ukf_batch_pda.h, DESIGN.md 4.30.
//
// Layout, LDS map (sensor_map), device functions and the statements up to the candidate loop are the association kernel's:
// one filter per 16-lane DPP row, chol(Sigma) and the sigma pair once, assoc_measure once (z-bar, S = Ls Ls^T, the lane's row of
// Y = C Ls^-T), candidates streamed with row-uniform addresses.  What differs:
//  * the normaliser A = ln(sum_{0, G} exp a) is known after the last candidate only.  The loop keeps RUNNING SUMS relative to a
//    running maximum mx of the exponents, which starts at a_0 (the "none of them" term, sum = 1): sum e, sum e y, sum e nu,
//    sum e y y^T with e = exp(a_k - mx).  When a candidate raises the maximum the sums are rescaled by exp(mx_old - mx_new),
//    else the candidate enters with exp(a_k - mx): ONE exponential per gated candidate, whichever way.  No exponent is ever
//    positive, so nothing overflows for any lambda, and sum >= 1;
//  * after the loop: A = mx + ln sum, beta_0 = exp(a_0 - A), y-bar, nu-bar and sum beta y y^T by one division, P_y, and the
//    middle matrix M = (1 - beta_0) I - P_y (symmetric, six values; columns of Y beyond m are zero, so I_3 serves I_m);
//  * Sigma~ = Sigma - Y M Y^T is not a product of three factors: the lane forms its row of W = Y M in registers (nine fma) and
//    runs the association's sg[c] loop with that row against Y's rows in LDS; delta = Y y-bar;
//  * beta_k = exp(a_k - A) needs A: a SECOND, cheap pass over z[k] recomputes y_k (pda_score, the same statements as the first
//    pass: the same bits) and stores beta.  The same pass rewrites the streamed scores of a filter whose Sigma~ failed
//    (ERR_CHOLESKY: all float outputs NaN); a wave-uniform branch skips it when no beta is wanted and no row failed there.
// A filter that fails, is gated, inactive or uninitialised rides along: every select is per row, no row's bits depend on its
// wave-mates.  commit = 0: the kernel gets NULL for the state's output pointers.
#pragma once

#include "ukf_associate.hpp"

namespace ukfb {

template <class T, class TS> struct PdaArgs {
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
    T gate_chi2;                 // < 0: every finite candidate is inside
    T a0_m1, a0_m3;              // ln lambda_m + ln(1 - P_D P_G,m) for m = 1 / m = 3
    T ln_pd;                     // ln P_D
    TS* z_pred;                  // [n][3] or null
    TS* S;                       // [n][9] or null
    TS* innov;                   // [candidates][n][3] or null
    TS* maha;                    // [candidates][n] or null
    TS* loglik;                  // [candidates][n] or null
    TS* beta;                    // [candidates][n] or null
    TS* beta0;                   // [n] or null
    TS* innov_comb;              // [n][3] or null
    int32_t* best;               // [n] or null
    int32_t* n_gated;            // [n] or null
    uint32_t* status;            // [n] or null
};

// One candidate against the row's hypothesis: nu = z - z-bar, y = Ls^-1 nu, d^2 = |y|^2.  Both passes call it.
template <class T> struct PdaScore {
    T nu[3], y[3], d2;
    bool present;
};
template <class T, class TS> UKFB_DEV PdaScore<T> pda_score(const TS* z, int64_t slot, int m, const AssocHyp<T>& hy) {
    PdaScore<T> s;
    T zk[3];
    s.present = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T v = T(z[slot * 3 + c]);
        s.present = s.present && (c >= m || m_finite(v));
        zk[c] = v;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T zin = T(double((c < m && s.present) ? zk[c] : T(0)) - hy.z0[c]);   // z - Z_0 (beyond m: 0 - 0)
        s.nu[c] = zin - hy.ref[c];
        s.y[c] = s.nu[c];
    }
    sensor_solve3(s.y, hy.l10, hy.l20, hy.l21, hy.rs);
    s.d2 = fma(s.y[0], s.y[0], fma(s.y[1], s.y[1], s.y[2] * s.y[2]));
    return s;
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_pda_kernel(const PdaArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2;
    constexpr SensorMap LY = sensor_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(2 * D * ZS <= LY.MUF - LY.TAB && SENSOR_INPUT_SCALARS <= LY.DUM - LY.INP, "W, Y and the input record fit their regions");
    extern __shared__ __attribute__((aligned(16))) unsigned char pda_smem[];

    const RowCoords<M> rc(a.n, threadIdx.x);
    const int l = rc.l, lr = rc.lr, ls = rc.ls;
    const bool fvalid = rc.fvalid;
    const int64_t f = rc.f;
    T* const base = row_slice<T, LY.PF>(pda_smem, rc.g);
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

    UKFB_MARK("p_sigma");
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

    UKFB_MARK("p_measure");
    // ================================================================= 2 - 4. z-bar, S = Ls Ls^T, Y = C Ls^-T: once
    AssocHyp<T> hy;
    assoc_measure<T, M>(xp, xm, id, m, hin, need_fwd, need_point, need_sens, do_0 && ok1, a.mean_tol, a.mean_max_it, FAC, INP, WT, DUMP, l, lr, hy);

    UKFB_MARK("p_candidates");
    // ================================================================= 5. per candidate: the scores and the running sums
    const T nanv = m_nan<T>();
    const T m_ln2pi = T(m) * T(1.8378770664093454835606594728112);
    const bool gate_on = !(a.gate_chi2 < T(0));
    const T a0 = (m == 1) ? a.a0_m1 : a.a0_m3;
    const T a_off = a.ln_pd - T(0.5) * (hy.lndet + m_ln2pi);   // a_k = a_off - d^2_k / 2
    const bool can_score = do_0 && ok1 && hy.ok2;
    T mx = a0, se = T(1);                                      // the "none of them" term
    T sy[3] = {T(0), T(0), T(0)}, snu[3] = {T(0), T(0), T(0)}, syy[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    T best_d2 = T(0);
    int best = -1, n_gated = 0;
    bool any_present = false, any_finite = false;
#pragma nounroll
    for (int k = 0; k < a.candidates; ++k) {
        const int64_t slot = int64_t(k) * a.n + f;
        const PdaScore<T> sc = pda_score<T, TS>(a.z, slot, m, hy);
        const bool scored = can_score && sc.present;
        const bool finite = scored && m_finite(sc.d2);
        const bool inside = finite && (!gate_on || sc.d2 <= a.gate_chi2);
        const bool better = inside && (best < 0 || sc.d2 < best_d2);   // equal d^2: the lower index stays
        any_present = any_present || sc.present;
        any_finite = any_finite || finite;
        n_gated += inside ? 1 : 0;
        best = better ? k : best;
        best_d2 = better ? sc.d2 : best_d2;
        {
            const T ak = fma(T(-0.5), sc.d2, a_off);
            const T dk = inside ? (ak - mx) : T(0);
            const T t = m_exp(-m_abs(dk));
            const bool up = dk > T(0);
            const T keep = up ? t : T(1);                      // the sums so far, relative to the new maximum
            const T e = inside ? (up ? T(1) : t) : T(0);       // this candidate
            mx = up ? ak : mx;
            se = fma(se, keep, e);
            T yk[3], nuk[3];   // (selects: y of a candidate that is not finite never meets the sums)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                yk[c] = inside ? sc.y[c] : T(0);
                nuk[c] = inside ? sc.nu[c] : T(0);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const T ey = e * yk[c];
                sy[c] = fma(sy[c], keep, ey);
                snu[c] = fma(snu[c], keep, e * nuk[c]);
#pragma unroll
                for (int d = 0; d <= c; ++d) syy[c * (c + 1) / 2 + d] = fma(syy[c * (c + 1) / 2 + d], keep, ey * yk[d]);
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
    const bool do_u = do_0 && any_present;
    const bool accept = n_gated > 0;

    UKFB_MARK("p_combine");
    // ================================================================= 6. A, beta_0, y-bar, nu-bar, M = (1 - beta_0) I - P_y
    const T lnA = mx + m_log(se);
    const T beta0 = m_exp(a0 - lnA);
    T yb[3], nub[3], m6[6];
    {
        const T inv = T(1) / se;
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
                m6[c * (c + 1) / 2 + d] = ((c == d) ? (T(1) - beta0) : T(0)) - py;
            }
    }
    T cr[3], wr[3];   // the lane's rows of Y and of W = Y M; no gated candidate: both zero
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
    UKFB_MARK("p_cov");
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
    UKFB_MARK("p_commit");
    // ================================================================= 8. commit: applyDelta(mu, Sigma~, delta)
    T mnew[S];
    const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mnew);
    const bool okc = ok1 && any_scored && (!accept || ok3);
    const bool good = do_u && okc && accept;
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!mvalid ? ST_INACTIVE : ((bad || !any_present) ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && ok1 && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && any_finite && !accept) ? ST_REJECTED_GATE : 0u;

    UKFB_MARK("p_store");
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
            if (a.best) a.best[f] = scored_f ? best : -1;
            if (a.n_gated) a.n_gated[f] = scored_f ? n_gated : 0;
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
    // ---- the second pass: beta_k = exp(a_k - A) from the recomputed y_k; a filter whose Sigma~ failed: the scores streamed above
    // become NaN (store-only; no row reads them)
    const bool undo = fvalid && do_u && any_scored && ok1 && accept && !ok3;
    if (a.beta != nullptr || wave_any(undo)) {
#pragma nounroll
        for (int k = 0; k < a.candidates; ++k) {
            const int64_t slot = int64_t(k) * a.n + f;
            const PdaScore<T> sc = pda_score<T, TS>(a.z, slot, m, hy);
            const bool scored = scored_f && sc.present;
            const bool finite = scored && m_finite(sc.d2);
            const bool inside = finite && (!gate_on || sc.d2 <= a.gate_chi2);
            const T bk = m_exp(fma(T(-0.5), sc.d2, a_off) - lnA);
            sfence();
            if (fvalid && l == 0 && a.beta) a.beta[slot] = TS(finite ? (inside ? bk : T(0)) : nanv);
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
