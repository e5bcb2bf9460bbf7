// ukf_delayed_chain.inc.hpp -- steps 1-2 of the delayed update, as statements: the backward chain from the engine's present state
// down to each row's step, with the operator M carried along it.  Included INSIDE a kernel body (no include guard), by
// ukf_delayed_kernel, by ukf_relative_kernel and by ukf_delayed_sensor_kernel: one statement of the chain, and the delayed kernel compiles the token stream it
// always had (as a shared function the same statements moved its register count).  The including body provides
//   a             the DelayedArgs<T, TS>
//   delayed_smem  the workgroup's dynamic LDS
//   st, chain_ok  uint32_t / bool, ST_OK / true on entry: the chain's statuses, and whether the row's chain is whole
//   ChainSample   a type with ChainSample(a, f, live).reach, the row's number of backward steps
// and the constants S, D, N = 2 D + 1, PK, LY (a map that extends delayed_map), LS, RT.  On exit the row's slice holds the
// smoothed past record in CSM / CSP and M in MOP; everything else in it is dead.
    int slot = a.top_slot;
    {
        // ---- the chain's start: the engine's own state, and M = I
        const DelayedRow<T, M, TS> r(a, delayed_smem, threadIdx.x);
        r.CSM[r.l] = T(a.mu[r.f * S + r.ls]);
        for (int i = r.l; i < PK; i += 16) r.CSP[i] = T(a.cov[r.f * PK + i]);
#pragma unroll
        for (int c = 0; c < D; ++c) r.MOP[r.lr * LS + c] = (c == r.lr) ? T(1) : T(0);   // (lanes >= D: row D - 1's own bits again)
        wsync();
    }
#pragma nounroll
    for (int k = 0; k < a.back; ++k) {
        // (the lane index passes through an opaque move in every step and its derivatives are formed again: ukf_smooth.hpp)
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        const DelayedRow<T, M, TS> row(a, delayed_smem, lane);
        const auto& [l, lr, ls, fvalid, live, f, FAC, RSP, TAB, GM, MM, CSM, CSP, MUF, PKF, ROT, DUMP, SMR, MUP, MOP, Rn, Racc] = row;
        int reach;
        {
            const ChainSample smp(a, f, live);
            reach = smp.reach;
        }
        if (!wave_any(k < reach)) break;   // the wavefront's largest lag is reached
        slot = (slot == 0) ? (a.slots - 1) : (slot - 1);
        const int64_t rec = int64_t(slot) * a.n + f;
        // ---- the filtered record of this step and its inputs
        MUF[l] = T(a.mu_hist[rec * S + ls]);
        for (int i = l; i < PK; i += 16) PKF[i] = T(a.cov_hist[rec * PK + i]);
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
        const double dt = a.dt[k];
        const bool neg = dt < 0.0, small = dt <= a.min_dt, large = dt > a.max_dt;
        const uint32_t code = neg ? ST_ERR_NEG_DT : (small ? ST_SKIPPED_SMALL_DT : (large ? ST_ERR_DT_TOO_LARGE : 0u));
        const bool inchain = k < reach;         // (reach > 0 only for rows that take part)
        st |= inchain ? code : 0u;
        const bool dof = inchain && chain_ok && code == 0u;   // a gated step passes chain and M through; so does a frozen row
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
            UKFB_MARK("d_predict");
            // ================================================================= 1. the prediction, redone (ukf_smooth.hpp)
            T mu_r[S], xp[S], xm[S], ref[S];
#pragma unroll
            for (int s = 0; s < S; ++s) mu_r[s] = MUF[s];
            {
                T q[4], rot[9];
                M::orientation(mu_r, q);
                quat_to_matrix(q, rot);
                T* dst = (l == 0) ? ROT : DUMP;
#pragma unroll
                for (int c = 0; c < 9; ++c) dst[c] = rot[c];
            }
            bool ok1;
            {
                T arow[D];
                load_row<T, D>(PKF, l, arow);
                const T rs = chol16<T, D, LS>(arow, FAC, l, ok1);
                wsync();
                row_scale_factor<T, D, LS>(FAC, RSP, l, rs);
                T col[D];
                load_column<T, D, LS>(FAC, l, T(1), col);
                sigma_pair<T, M>(mu_r, col, xp, xm);
            }
            sfence();
            process_fast((M*)nullptr, xp, pin);
            sfence();
            process_fast((M*)nullptr, xm, pin);
            sfence();
#pragma unroll
            for (int s = 0; s < S; ++s) ref[s] = row_bcast<D>(xp[s]);
            bool conv = true;
            {
                const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
                bool active = dof && ok1;
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
            row_publish_deltas<T, M, LS>(TAB, DUMP, l, xp, xm, ref);
            wsync();
            T sm[D];
            row_table_row<T, D, LS>(TAB, N, lr, sm);
            sfence();
#pragma unroll
            for (int c = 0; c < D; ++c) SMR[lr * LS + c] = sm[c];
            sfence();
#pragma nounroll
            for (int c = 0; c < D; ++c) {
                const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
                const T nz = (c < 6) ? process_noise_entry16<T, M, TS>(Rn, Racc, ROT, pin, hi, lo)
                                     : plain_noise_entry16<T, M, TS>(Rn, Racc, pin, hi, lo);
                SMR[lr * LS + c] += nz;
            }
            {
                T* dst = (l == 0) ? MUP : DUMP;
#pragma unroll
                for (int s2 = 0; s2 < S; ++s2) dst[s2] = ref[s2];
            }
            sfence();
            UKFB_MARK("d_cross");
            // ================================================================= 2. C, 3. G = C (Sigma^-)^-1
            T g_[D];
            {
                T cr[D];
#pragma unroll
                for (int c = 0; c < D; ++c) cr[c] = T(0);
#pragma nounroll
                for (int j = 0; j < D; ++j) {
                    const T lj = FAC[j * LS + lr];
                    const T* w = TAB + (D + j) * LS;
#pragma unroll
                    for (int c = 0; c < D; ++c) cr[c] = fma(lj, w[c], cr[c]);
                }
                wsync();
                bool ok2;
                {
                    T tmp[D];
#pragma unroll
                    for (int c = 0; c < D; ++c) tmp[c] = SMR[lr * LS + c];
                    const T rs = chol16<T, D, LS>(tmp, FAC, l, ok2);
                    wsync();
                    row_scale_factor<T, D, LS>(FAC, RSP, l, rs);
                }
                ok1 = ok1 && ok2;
#pragma unroll
                for (int k2 = 0; k2 < D; ++k2) {
                    T v = cr[k2];
#pragma unroll
                    for (int j = 0; j < k2; ++j) v = fma(-FAC[j * LS + k2], cr[j], v);
                    cr[k2] = v * RSP[k2];
                    sfence();
                }
#pragma unroll
                for (int k2 = D - 1; k2 >= 0; --k2) {
                    T v = cr[k2];
#pragma unroll
                    for (int j = k2 + 1; j < D; ++j) v = fma(-FAC[k2 * LS + j], cr[j], v);
                    cr[k2] = v * RSP[k2];
                    sfence();
                }
#pragma unroll
                for (int c = 0; c < D; ++c) g_[c] = cr[c];
            }
            wsync();
#pragma unroll
            for (int c = 0; c < D; ++c) GM[lr * LS + c] = g_[c];
            UKFB_MARK("d_transport");
            // ================================================================= 4. transport of the chain to the tangent space at mu^-
            T e[D];
            {
                T cs[S], mp[S];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    cs[s] = CSM[s];
                    mp[s] = MUP[s];
                }
                row_boxminus<T, M>(cs, mp, e);
            }
            const int li = lr - RT;
            const bool inrot = li >= 0 && li < 3;
            {
                const T ph[3] = {e[RT], e[RT + 1], e[RT + 2]};
                const T t = fma(ph[0], ph[0], fma(ph[1], ph[1], ph[2] * ph[2]));
                T B[9];
                delayed_rot_matrix(ph, t, T(0.5), bank_jrinv_coeff(t), B);
                T s[D];
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
                    s[c] = CSP[hi * (hi + 1) / 2 + lo];
                }
                {
                    const T s0 = s[RT], s1 = s[RT + 1], s2 = s[RT + 2];
#pragma unroll
                    for (int i = 0; i < 3; ++i) s[RT + i] = fma(s0, B[3 * i], fma(s1, B[3 * i + 1], s2 * B[3 * i + 2]));
                }
                const T b0 = (li == 1) ? B[3] : ((li == 2) ? B[6] : B[0]);
                const T b1 = (li == 1) ? B[4] : ((li == 2) ? B[7] : B[1]);
                const T b2 = (li == 1) ? B[5] : ((li == 2) ? B[8] : B[2]);
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const T r0 = row_bcast<RT>(s[c]), r1 = row_bcast<RT + 1>(s[c]), r2 = row_bcast<RT + 2>(s[c]);
                    const T rot = fma(b0, r0, fma(b1, r1, b2 * r2));
                    MM[lr * LS + c] = (inrot ? rot : s[c]) - SMR[lr * LS + c];
                }
                // ============================================================= 4b. row lr of G J: the rotation columns of G times Jr^-1,
                // through the dead factor region (the product below indexes it by a loop variable)
                {
                    const T g0 = g_[RT], g1 = g_[RT + 1], g2 = g_[RT + 2];
#pragma unroll
                    for (int i = 0; i < 3; ++i) g_[RT + i] = fma(g0, B[i], fma(g1, B[3 + i], g2 * B[6 + i]));
                }
#pragma unroll
                for (int c = 0; c < D; ++c) FAC[lr * LS + c] = g_[c];
            }
            wsync();
            UKFB_MARK("d_operator");
            // ================================================================= 4c. M <- A (G J) M: row lr
            {
                T tr[D];
#pragma unroll
                for (int c = 0; c < D; ++c) tr[c] = T(0);
#pragma nounroll
                for (int j = 0; j < D; ++j) {
                    const T gj = FAC[lr * LS + j];
                    const T* mrow = MOP + j * LS;
#pragma unroll
                    for (int c = 0; c < D; ++c) tr[c] = fma(gj, mrow[c], tr[c]);
                }
                // delta = G e (its rotation part: A's argument)
                T dl = T(0);
#pragma unroll
                for (int c = 0; c < D; ++c) dl = fma(GM[lr * LS + c], e[c], dl);
                const T dr[3] = {row_bcast<RT>(dl), row_bcast<RT + 1>(dl), row_bcast<RT + 2>(dl)};
                const T t = fma(dr[0], dr[0], fma(dr[1], dr[1], dr[2] * dr[2]));
                T ja, jb, A[9];
                delayed_jr_coeffs(t, ja, jb);
                delayed_rot_matrix(dr, t, -ja, jb, A);
                const T a0 = (li == 1) ? A[3] : ((li == 2) ? A[6] : A[0]);
                const T a1 = (li == 1) ? A[4] : ((li == 2) ? A[7] : A[1]);
                const T a2 = (li == 1) ? A[5] : ((li == 2) ? A[8] : A[2]);
                wsync();   // every lane has read the rows of M
                T* const dst = dof ? (MOP + lr * LS) : DUMP;   // a frozen, gated or broken row keeps its M
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const T r0 = row_bcast<RT>(tr[c]), r1 = row_bcast<RT + 1>(tr[c]), r2 = row_bcast<RT + 2>(tr[c]);
                    const T rot = fma(a0, r0, fma(a1, r1, a2 * r2));
                    dst[dof ? c : 0] = inrot ? rot : tr[c];
                }
            }
            wsync();
            UKFB_MARK("d_cov");
            // ================================================================= 5. Sigma~ = Sigma + (G M) G^T: row lr, and delta = G e
            T sg[D], del[D];
            {
                T tr[D];
#pragma unroll
                for (int c = 0; c < D; ++c) tr[c] = T(0);
#pragma nounroll
                for (int j = 0; j < D; ++j) {
                    const T gj = GM[lr * LS + j];
                    const T* m = MM + j * LS;
#pragma unroll
                    for (int c = 0; c < D; ++c) tr[c] = fma(gj, m[c], tr[c]);
                }
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
                    sg[c] = PKF[hi * (hi + 1) / 2 + lo];
                }
#pragma unroll
                for (int c = 0; c < D; ++c) FAC[lr * LS + c] = tr[c];
                sfence();
#pragma nounroll
                for (int j = 0; j < D; ++j) {
                    const T tj = FAC[lr * LS + j];
                    const T* gc = GM + j;
#pragma unroll
                    for (int c = 0; c < D; ++c) sg[c] = fma(tj, gc[c * LS], sg[c]);
                }
                sfence();
                T dl = T(0);
#pragma unroll
                for (int c = 0; c < D; ++c) dl = fma(GM[lr * LS + c], e[c], dl);
                static_for<0, D>([&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    del[c] = row_bcast<c>(dl);
                });
            }
            wsync();
            UKFB_MARK("d_commit");
            // ================================================================= 6. commit: applyDelta(mu, Sigma~, delta)
            bool ok3;
            T mnew[S];
            {
                const T rs = chol16<T, D, LS>(sg, FAC, l, ok3);
                wsync();
                T col[D], dpl[D], dmi[D];
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
            bool inf = false;   // (the chain must stay finite: an Inf that the factorisations let through would poison M)
#pragma unroll
            for (int c = 0; c < D; ++c) inf = inf || !m_finite(sg[c]);
            const bool good = dof && ok1 && ok3 && !row_any(inf);
            st |= (dof && !good) ? ST_ERR_CHOLESKY : 0u;
            st |= (dof && good && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
            chain_ok = chain_ok && !(dof && !good);   // a broken chain refuses the sample
            {
                T v = mnew[0];
#pragma unroll
                for (int s = 1; s < S; ++s) v = (ls == s) ? mnew[s] : v;
                T* dst = (good && l < S) ? (CSM + l) : DUMP;
                *dst = v;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const int idx = lr * (lr + 1) / 2 + c;
                    const bool own = good && l < D && c <= l;
                    T* dc = own ? (CSP + idx) : DUMP;
                    *dc = sg[c];
                }
            }
            wsync();
        }
    }
