// ukf_delayed_retro.inc.hpp -- steps 3d-5 of the delayed update, as statements: C_z against the factor of Sigma^s, the 3 x 3 factor of
// S in registers, Y_s, the retrodiction Y_n = Sigma_n M^T (Sigma^s)^-1 Y_s, Sigma~_n, the commit applyDelta(mu_n, Sigma~_n, Y_n y)
// and the call's status.  Included INSIDE a kernel body (no include guard), by ukf_delayed_kernel and by ukf_delayed_sensor_kernel
// (ukf_delayed_sensor.hpp), as the chain is (ukf_delayed_chain.inc.hpp): one statement of every step, and the delayed kernel
// compiles the token stream it always had.  The including body provides, after its own mean and statistics,
//   a, st, chain_ok, ok1, conv, do_u, fvalid, live, smp (.inactive, .old, .bad), m
//   s6 (S packed, the identity beyond m), nu, and W in WT; the row's l, lr, ls and its regions FAC, RSP, TAB, WT, YM, YN, MOP,
//   MUF, PKF (the present state), DUMP; the constants S, D, PK, LS, ZS
// and finds on exit mnew / sg published in TAB's row 2 D, ok2, ok3, okc, good, accept, d2, lndet, yn.
    UKFB_MARK("d_cross_z");
    // ================================================================= 3d. C_z row lr, S = Ls Ls^T in registers, Y_s = C_z Ls^-T, y = Ls^-1 nu
    bool ok2;
    T lndet, d2, yn[3];
    {
        T cr[3] = {T(0), T(0), T(0)};
#pragma nounroll
        for (int j = 0; j < D; ++j) {
            const T lj = FAC[j * LS + lr];
            const T* w = WT + j * ZS;
#pragma unroll
            for (int c = 0; c < 3; ++c) cr[c] = fma(lj, w[c], cr[c]);
        }
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
        T* const dst = (l < D) ? (YM + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = cr[c];
    }
    const bool accept = (a.gate_chi2 < T(0)) || (d2 <= a.gate_chi2);
    wsync();
    UKFB_MARK("d_retro");
    // ================================================================= 4. Y_n = Sigma_n M^T (Sigma^s)^-1 Y_s: row lr
    T yr[3] = {T(0), T(0), T(0)};
    {
        T nr[D];
#pragma unroll
        for (int c = 0; c < D; ++c) nr[c] = T(0);
#pragma nounroll
        for (int j = 0; j < D; ++j) {   // N[lr][c] = sum_j Sigma_n[lr][j] M[c][j]
            const int hi = lr > j ? lr : j, lo = lr > j ? j : lr;
            const T sj = PKF[hi * (hi + 1) / 2 + lo];
            const T* mc = MOP + j;
#pragma unroll
            for (int c = 0; c < D; ++c) nr[c] = fma(sj, mc[c * LS], nr[c]);
        }
        // P = N (Sigma^s)^-1: the smoother's two triangular solves per row, against the factor of Sigma^s
#pragma unroll
        for (int k2 = 0; k2 < D; ++k2) {
            T v = nr[k2];
#pragma unroll
            for (int j = 0; j < k2; ++j) v = fma(-FAC[j * LS + k2], nr[j], v);
            nr[k2] = v * RSP[k2];
            sfence();
        }
#pragma unroll
        for (int k2 = D - 1; k2 >= 0; --k2) {
            T v = nr[k2];
#pragma unroll
            for (int j = k2 + 1; j < D; ++j) v = fma(-FAC[k2 * LS + j], nr[j], v);
            nr[k2] = v * RSP[k2];
            sfence();
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const T* ys = YM + j * ZS;
#pragma unroll
            for (int c = 0; c < 3; ++c) yr[c] = fma(nr[j], ys[c], yr[c]);
        }
        T* const dst = (l < D) ? (YN + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = yr[c];
    }
    wsync();
    UKFB_MARK("d_cov_n");
    // ================================================================= 5. Sigma~_n = Sigma_n - Y_n Y_n^T: row lr, and delta = Y_n y
    T sg[D], del[D];
    {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T* yc = YN + c * ZS;   // the rows other lanes wrote
            sg[c] = fma(-yr[2], yc[2], fma(-yr[1], yc[1], fma(-yr[0], yc[0], PKF[hi * (hi + 1) / 2 + lo])));
        }
        const T dl = fma(yr[2], yn[2], fma(yr[1], yn[1], yr[0] * yn[0]));
        static_for<0, D>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            del[c] = row_bcast<c>(dl);
        });
    }
    wsync();   // W, Y_s, Y_n and the factor of Sigma^s are dead
    UKFB_MARK("d_commit_n");
    bool ok3;
    T mnew[S];
    {
        const T rs = chol16<T, D, LS>(sg, FAC, l, ok3);
        wsync();
        T col[D], dpl[D], dmi[D], mu_r[S], xp[S], xm[S];
        load_column<T, D, LS>(FAC, l, rs, col);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            dpl[c] = del[c] + col[c];
            dmi[c] = del[c] - col[c];
        }
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) mu_r[s2] = MUF[s2];
        sfence();
        row_boxplus<T, M>(mu_r, del, mnew);
        row_boxplus<T, M>(mu_r, dpl, xp);
        row_boxplus<T, M>(mu_r, dmi, xm);
        row_publish_deltas<T, M, LS>(TAB, DUMP, l, xp, xm, mnew);
    }
    wsync();
    row_table_row<T, D, LS>(TAB, 2 * D, lr, sg);
    bool inf = false;
#pragma unroll
    for (int c = 0; c < D; ++c) inf = inf || !m_finite(sg[c]);
    const bool fin = !row_any(inf);
    const bool okc = chain_ok && ok1 && ok2 && (!accept || (ok3 && fin));
    const bool good = do_u && okc && accept;
    st |= !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (smp.inactive ? ST_INACTIVE : (smp.old ? ST_ERR_NEG_DT : (smp.bad ? ST_ERR_NONFINITE_MEAS : ST_OK))));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && chain_ok && ok1 && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && !accept) ? ST_REJECTED_GATE : 0u;
