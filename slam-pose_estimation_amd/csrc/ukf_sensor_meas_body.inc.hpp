// ukf_sensor_meas_body.inc.hpp -- the sensor-frame update of one workgroup, as statements.  Included INSIDE a kernel body (no
// include guard), by ukf_sensor_meas_kernel and by ukf_robust_kernel (ukf_robust.hpp): one statement of every step, and the
// sensor kernel compiles the token stream it always had (as a shared device function behind two thin kernels the same statements
// moved its register count from 210 to 211 and reordered its argument loads).  The including kernel provides
//   T, M, TS   compute type, model over it, storage type
//   a          SensorArgs<T, TS>, or RobustArgs<T, TS>: then ROBUST is true, and what stands under `if constexpr (ROBUST)`
//              keeps Q apart from Sigma_z, asks robust_scale for lambda and forms S(lambda) before step 6
// The factorisation and the commit below are the statements of row_factorise / row_apply_delta (ukf_row.hpp) in place: built
// on them this kernel left the spread of the parent's own runs (profiles/row_toolkit_rates.txt), so it keeps them as tuned.
    constexpr bool ROBUST = sensor_args_robust<std::remove_cv_t<decltype(a)>>;
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr SensorMap LY = sensor_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(2 * D * ZS <= LY.MUF - LY.TAB && SENSOR_INPUT_SCALARS <= LY.DUM - LY.INP, "W, Y and the input record fit their regions");
    extern __shared__ __attribute__((aligned(16))) unsigned char sen_smem[];

    // (RowCoords' statements in place: built on it, this kernel left the spread of the parent's own runs -- profiles/row_toolkit_rates.txt)
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int lr = (l < D) ? l : (D - 1), ls = (l < S) ? l : (S - 1);
    const int64_t wg0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * ROW_FILTERS_PER_GROUP;
    const int64_t n_here = a.n - wg0;
    const int n_wg = int(n_here < ROW_FILTERS_PER_GROUP ? n_here : int64_t(ROW_FILTERS_PER_GROUP));
    const bool fvalid = g < n_wg;
    const int64_t f = wg0 + (fvalid ? g : (n_wg - 1));   // rows beyond the batch repeat its last filter and store nothing
    T* const base = reinterpret_cast<T*>(sen_smem) + g * LY.PF;
    T *const FAC = base + LY.FAC, *const RSP = base + LY.RSP, *const TAB = base + LY.TAB, *const WT = base + LY.WT;
    T *const YM = base + LY.YM, *const MUF = base + LY.MUF, *const PKF = base + LY.PKF, *const INP = base + LY.INP;
    T* const DUMP = base + LY.DUM;

    // ---- the row's filter, model and records
    const bool live = fvalid && a.initialised[f] != 0;
    const int mid = a.model ? a.model[f] : a.model_uniform;
    const bool mvalid = sensor_model_ok(M::MODEL, int64_t(mid));
    const int id = mvalid ? mid : (M::MODEL == 0 ? int(UKFB_SENSOR_POSE_POSITION) : int(UKFB_SENSOR_ORIENT_VELOCITY));   // no valid id: the row rides along
    const int m = sensor_meas_dim(id);
    MUF[l] = T(a.mu[f * S + ls]);
    for (int i = l; i < PK; i += 16) PKF[i] = T(a.cov[f * PK + i]);
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
            src = is_z ? (a.z + f * 3 + i) : src;
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
            const bool used = sensor_input_used(int64_t(id), i);
            b = b || (used && !m_finite(v));
            INP[i] = used ? v : ((i == SENSOR_INPUT_MOUNT + 6) ? T(1) : T(0));
        }
        bad = row_any(b);
    }
    wsync();
    const bool do_u = live && mvalid && !bad;

    UKFB_MARK("n_sigma");
    // ================================================================= 1. sigma points of (mu, Sigma)
    // h, and the differences of its values to the centre's, are evaluated in fp64 in every mode: a beacon tens of metres away puts
    // an ulp of 4e-6 m on everything h forms in fp32, against innovations of centimetres
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
        T arow[D];
        load_row<T, D>(PKF, l, arow);
        const T rs = chol16<T, D, LS>(arow, FAC, l, ok1);
        wsync();
        row_scale_factor<T, D, LS>(FAC, RSP, l, rs);   // the scaled columns stay: C reads them
        T col[D];
        load_column<T, D, LS>(FAC, l, T(1), col);
        sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: the centre twice (their column is zero)
    }
    sfence();
    UKFB_MARK("n_measure");
    // ================================================================= 2. Z = h(X) on the lane's pair, relative to Z_0
    // From here on the measurement side works in coordinates whose origin is Z_0: the mean iteration, the deltas and the innovation
    // are differences of differences to the centre.  On a vector space that is the same iteration (it is translation invariant),
    // but its iterate is a small number: in fp32 a z-bar of tens of metres has half an ulp above mean_tol, and the iteration in
    // absolute coordinates would neither converge nor resolve the deltas.
    T zp[3], zm[3], zin[3], ref[3] = {T(0), T(0), T(0)};
    TH z0[3];
    {
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
    UKFB_MARK("n_mean");
    // ================================================================= 3. z-bar - Z_0: ukfom's iterated mean on R^3
    bool conv = true;
    const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
    {
        bool active = do_u && ok1;
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
    UKFB_MARK("n_stats");
    // ================================================================= 4. S = 1/2 sum dz dz^T + Q (identity beyond m), nu, W to LDS
    T s6[6], nu[3], zbar[3];
    T q6[6];   // ROBUST: Q apart from Sigma_z
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
                if constexpr (ROBUST) {   // s6 = Sigma_z until lambda is known
                    q6[r * (r + 1) / 2 + c] = (r < m) ? q : T(0);
                    s6[r * (r + 1) / 2 + c] = (r < m) ? s6[r * (r + 1) / 2 + c] : ((r == c) ? T(1) : T(0));
                } else
                    s6[r * (r + 1) / 2 + c] = (r < m) ? (s6[r * (r + 1) / 2 + c] + q) : ((r == c) ? T(1) : T(0));   // (c <= r < m)
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            nu[c] = zin[c] - ref[c];
            zbar[c] = T(z0[c] + TH(ref[c]));
        }
    }
    wsync();
    UKFB_MARK("n_cross");
    // ================================================================= 5. C = sum_j (L col j) W_j^T: row lr
    T cr[3] = {T(0), T(0), T(0)};
#pragma nounroll
    for (int j = 0; j < D; ++j) {
        const T lj = FAC[j * LS + lr];
        const T* w = WT + j * ZS;
#pragma unroll
        for (int c = 0; c < 3; ++c) cr[c] = fma(lj, w[c], cr[c]);
    }
    RobustScale<T> rb{};
    if constexpr (ROBUST) {
        UKFB_MARK("n_scale");
        // ============================================================= lambda; then S(lambda) = Sigma_z + lambda Q, entry by entry
        rb = robust_scale(a, s6, q6, nu, m, do_u && ok1);
#pragma unroll
        for (int i = 0; i < 6; ++i) s6[i] = fma(rb.lam, q6[i], s6[i]);   // lambda = 1: Sigma_z + q to the bit; beyond m: 1 and 0
    }
    UKFB_MARK("n_solve");
    // ================================================================= 6. S = Ls Ls^T in registers; Y = C Ls^-T, y = Ls^-1 nu
    bool ok2;
    T lndet, d2, yn[3];
    {
        const T d0 = s6[0], i0 = fast_rcp(d0);
        const T t10 = s6[1] * i0, t20 = s6[3] * i0;
        const T d1 = fma(-t10, s6[1], s6[2]), a21 = fma(-t20, s6[1], s6[4]);
        const T i1 = fast_rcp(d1);
        const T d2p = fma(-(a21 * i1), a21, fma(-t20, s6[3], s6[5]));
        ok2 = (d0 > T(0)) && (d1 > T(0)) && (d2p > T(0));   // (NaN fails every comparison)
        lndet = m_log(d0) + m_log(d1) + m_log(d2p);          // a pivot beyond m is exactly 1
        const T rs[3] = {fast_rsqrt(d0), fast_rsqrt(d1), fast_rsqrt(d2p)};
        const T l10 = s6[1] * rs[0], l20 = s6[3] * rs[0], l21 = a21 * rs[1];
        sensor_solve3(cr, l10, l20, l21, rs);
#pragma unroll
        for (int c = 0; c < 3; ++c) yn[c] = nu[c];
        sensor_solve3(yn, l10, l20, l21, rs);
        d2 = fma(yn[0], yn[0], fma(yn[1], yn[1], yn[2] * yn[2]));
    }
    bool accept;
    if constexpr (ROBUST)
        accept = rb.accept;   // the gate acts on the raw distance
    else
        accept = (a.gate_chi2 < T(0)) || (d2 <= a.gate_chi2);
    {
        T* const dst = (l < D) ? (YM + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = cr[c];
    }
    wsync();
    UKFB_MARK("n_cov");
    // ================================================================= 7. Sigma~ = Sigma - Y Y^T: row lr, and delta = Y y
    T sg[D], del[D];
    {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T* yc = YM + c * ZS;   // the rows other lanes wrote
            sg[c] = fma(-cr[2], yc[2], fma(-cr[1], yc[1], fma(-cr[0], yc[0], PKF[hi * (hi + 1) / 2 + lo])));
        }
        const T dl = fma(cr[2], yn[2], fma(cr[1], yn[1], cr[0] * yn[0]));
        static_for<0, D>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            del[c] = row_bcast<c>(dl);
        });
    }
    wsync();   // W, Y and the factor of Sigma are dead
    UKFB_MARK("n_commit");
    // ================================================================= 8. commit: applyDelta(mu, Sigma~, delta)
    bool ok3;
    T mnew[S];
    {
        const T rs = chol16<T, D, LS>(sg, FAC, l, ok3);
        wsync();
        T col[D], dpl[D], dmi[D], mu_r[S];
        load_column<T, D, LS>(FAC, l, rs, col);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            dpl[c] = del[c] + col[c];
            dmi[c] = del[c] - col[c];
        }
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) mu_r[s2] = MUF[s2];   // (reloaded: not kept live across the kernel)
        sfence();
        row_boxplus<T, M>(mu_r, del, mnew);
        row_boxplus<T, M>(mu_r, dpl, xp);
        row_boxplus<T, M>(mu_r, dmi, xm);
        row_publish_deltas<T, M, LS>(TAB, DUMP, l, xp, xm, mnew);
    }
    wsync();
    row_table_row<T, D, LS>(TAB, 2 * D, lr, sg);
    const bool okc = ok1 && ok2 && (!accept || ok3);
    const bool good = do_u && okc && accept;
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!mvalid ? ST_INACTIVE : (bad ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && ok1 && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && !accept) ? ST_REJECTED_GATE : 0u;

    UKFB_MARK("n_store");
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
    if (good && a.mu_out) {
        if (l < S) a.mu_out[f * S + l] = TS(MUF[l]);
        for (int i = l; i < PK; i += 16) a.cov_out[f * PK + i] = TS(PKF[i]);
    }
    if (fvalid) {
        const bool scored = do_u && okc;
        const T nanv = m_nan<T>();
        if (l < 3) {
            T zb = zbar[0], iv = nu[0];
#pragma unroll
            for (int c = 1; c < 3; ++c) {
                zb = (l == c) ? zbar[c] : zb;
                iv = (l == c) ? nu[c] : iv;
            }
            if (a.z_pred) a.z_pred[f * 3 + l] = TS(scored ? ((l < m) ? zb : T(0)) : nanv);
            if (a.innov) a.innov[f * 3 + l] = TS((l < m) ? (scored ? iv : nanv) : T(0));
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
            if constexpr (ROBUST) {
                if (a.maha0) a.maha0[f] = TS(scored ? rb.d0sq : nanv);
                if (a.scale) a.scale[f] = TS(scored ? rb.lam : nanv);
                if (a.iterations) a.iterations[f] = scored ? rb.its : 0;
            }
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
