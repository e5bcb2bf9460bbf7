// ukf_relative.hpp -- relative measurements: an increment (R(q_s)^T (p_n - p_s), q_s^-1 q_n) between step s = n - lag of the
// history and the present, as odometry and scan matching report it.  The delayed update's backward chain gives the smoothed past
// state (mu^s_s, Sigma^s_s) and the regression M_s of x_s on x_n; ukfom's update is then made on the pair (x_n, x_s) -- the state
// augmented by a clone -- and only the present state is kept.  Definitions: include/ukf_batch_relative.h,
// DESIGN.md 4.27.  Pose engines only.
//
// Layout: the delayed kernel's (ukf_delayed.hpp) -- one filter per 16-lane row, four per wavefront, its chain
// (ukf_delayed_chain.inc.hpp) and
// its LDS slice; ONE kernel: everything the update adds lives in regions of that slice the chain leaves dead (relative_map).
//  * Sigma_e = Sigma^s_s - M Sigma_n M^T: lane l forms row l of N = Sigma_n M^T, parks it, and takes row l of M N (two row x
//    matrix products with broadcast reads), then the clamped factorisation L_e (relative_chol_clamped) beside L_n = chol(Sigma_n).
//    (L_n, 0; M L_n, L_e) is the lower factor of the joint covariance of (x_n, x_s) wherever no pivot is clamped.
//  * h reads positions and orientations only, so a sigma pair needs the first six rows of its columns: lane j < D takes column j
//    of L_n and of L_e from LDS and forms its six entries of column j of M L_n in registers (M L_n is never stored).
//  * lane j < D evaluates four points: (mu_n [+] +-L_n col j, mu^s_s [+] +-(M L_n) col j) and (mu_n, mu^s_s [+] +-L_e col j); lane D
//    the centre.  4 D + 1 points of weight 1 / (4 D + 1), the iterated mean on R^3 x SO(3), S (21 entries) on every lane by row
//    all-reductions, the 6 x 6 factor of S in registers.  A model that reads one part has the other part's deltas zeroed and
//    S = I there, so one code path serves m = 3 and m = 6.
//  * C_n row = sum_j L_n[l][j] W_j over the FIRST 2 D points, Y_n = C_n Ls^-T, Sigma~_n = Sigma_n - Y_n Y_n^T and the update's
//    own commit (row_apply_delta).
//  * TS (storage) / T (compute) as in ukf_delayed.hpp.  Plain fp32 holds the 1e-4 gate without any fp64 piece
//    (tests/test_relative_reference.py: the study of the all-float32 evaluation, the Sigma_e subtraction included).
#pragma once

#include "ukf_delayed.hpp"

namespace ukfb {

// The kernel's arguments are the delayed update's, field for field; what differs is the shape of the sample and of the scores:
// z [n][7] (dp, then dq as x y z w), Q [n][36] or [36], z_pred [n][7], S [n][36], innov [n][6].
template <class T, class TS> using RelativeArgs = DelayedArgs<T, TS>;

template <class T> struct RelativeEps;
template <> struct RelativeEps<double> { static constexpr double tau = 64.0 * 2.220446049250313e-16; };
template <> struct RelativeEps<float> { static constexpr float tau = 64.0f * 1.1920929e-7f; };

// What a row's increment asks for (the same from every lane of the row)
template <class T, class M, class TS> struct RelativeSample {
    int reach;
    bool selp, selq, inactive, old, bad, do_u;
    UKFB_DEV RelativeSample(const DelayedArgs<T, TS>& a, int64_t f, bool live) {
        const int mid = a.model ? a.model[f] : a.model_uniform;
        const int lag = a.lag ? a.lag[f] : a.lag_uniform;
        const bool mvalid = relative_model_ok(mid);
        selp = !mvalid || mid != UKFB_RELATIVE_ROTATION;
        selq = !mvalid || mid != UKFB_RELATIVE_POSITION;
        inactive = lag <= 0 || !mvalid;   // an increment over no steps measures nothing
        old = !inactive && lag > a.back;
        bool fin = true;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const T v = T(a.z[f * 7 + c]);
            const bool used = (c < 3) ? selp : selq;
            fin = fin && (!used || m_finite(v));
        }
        const TS* qp = a.Q + (a.q_uniform ? int64_t(0) : f * 36);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const bool used = ((r < 3) ? selp : selq) && ((c < 3) ? selp : selq);
                fin = fin && (!used || m_finite(T(qp[6 * r + c])));
            }
        bad = !fin;
        do_u = live && !inactive && !old && !bad;
        reach = do_u ? lag : 0;
    }
};

// the sample, the part a model does not read replaced by the neutral element (0, identity)
template <class T, class TS> UKFB_DEV void relative_load_sample(const DelayedArgs<T, TS>& a, int64_t f, bool selp, bool selq, T (&zin)[7]) {
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const T v = T(a.z[f * 7 + c]);
        zin[c] = ((c < 3) ? selp : selq) ? v : ((c == 6) ? T(1) : T(0));
    }
}

// Clamped factorisation of the lane's row `a` of a symmetric positive SEMIdefinite matrix (lower triangle): with x_k the pivot
// after its subtractions and a_kk the scale of row k, x_k > tau a_kk is an ordinary column, |x_k| <= tau a_kk a zero column (no
// trailing update), x_k < -tau a_kk (or a NaN) fails.  diag: the lane's a_ll -- the diagonal entry of the matrix `a` was formed
// from by subtraction (Sigma^s_s for Sigma_e): in a direction the present determines, the matrix's own entry is the rounding
// error of that subtraction, of either sign, and measures nothing.  Publishes the SCALED columns, zeros above the diagonal.
template <class T, int D, int LS> UKFB_DEV bool relative_chol_clamped(T (&a)[D], T diag, T* Lc, int l) {
    const int lw = (l < D) ? l : (D - 1);
    bool good = true;
    static_for<0, D>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        dpp_hazard_fence(a[k]);
        dpp_hazard_fence(diag);
        const T x = row_bcast<k>(a[k]);
        const T lim = RelativeEps<T>::tau * row_bcast<k>(diag);
        const bool pos = x > lim && m_finite(x);
        const bool zero = !pos && (m_abs(x) <= lim);   // (NaN fails both)
        good = good && (pos || zero);
        const T xs = pos ? x : T(1);
        const T rs = pos ? fast_rsqrt(xs) : T(0);
        Lc[k * LS + lw] = (l >= k) ? a[k] * rs : T(0);
        const T nt = -(a[k] * (rs * rs));
        if constexpr (k + 1 < D) {
            static_for<k + 1, D>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                fmac_bcast<c>(a[c], a[k], nt);
            });
        }
    });
    return good;
}

// S = L L^T of a symmetric 6 x 6 matrix in registers (packed lower triangle, in place); rs: the reciprocal diagonal of L
template <class T> UKFB_DEV void relative_chol6(T (&s)[21], T (&rs)[6], bool& ok, T& lndet) {
    ok = true;
    lndet = T(0);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        T x = s[k * (k + 1) / 2 + k];
#pragma unroll
        for (int j = 0; j < k; ++j) x = fma(-s[k * (k + 1) / 2 + j], s[k * (k + 1) / 2 + j], x);
        ok = ok && (x > T(0)) && m_finite(x);
        lndet += m_log(x);
        rs[k] = fast_rsqrt(x);
        s[k * (k + 1) / 2 + k] = x * rs[k];
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            T v = s[i * (i + 1) / 2 + k];
#pragma unroll
            for (int j = 0; j < k; ++j) v = fma(-s[i * (i + 1) / 2 + j], s[k * (k + 1) / 2 + j], v);
            s[i * (i + 1) / 2 + k] = v * rs[k];
        }
    }
}
// v <- L^-1 v (as a row: v <- v L^-T)
template <class T> UKFB_DEV void relative_solve6(T (&v)[6], const T (&L)[21], const T (&rs)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        T x = v[k];
#pragma unroll
        for (int j = 0; j < k; ++j) x = fma(-L[k * (k + 1) / 2 + j], v[j], x);
        v[k] = x * rs[k];
    }
}

// h(x_n, x_s) of the pair (p_n + dn[0:3], q_n exp(+-dn[3:6])), (p_s + ds[0:3], q_s exp(+-ds[3:6])): both signs at once
template <class T>
UKFB_DEV void relative_measure_pair(const T (&xn)[7], const T (&xs)[7], const T (&dn)[6], const T (&ds)[6], T (&zp)[7], T (&zm)[7]) {
    const T qn[4] = {xn[3], xn[4], xn[5], xn[6]}, qs[4] = {xs[3], xs[4], xs[5], xs[6]};
    const T vn[3] = {dn[3], dn[4], dn[5]}, vs[3] = {ds[3], ds[4], ds[5]};
    T en[4], es[4], qnp[4], qnm[4], qsp[4], qsm[4];
    so3_exp_fast(vn, T(1), en);
    so3_exp_fast(vs, T(1), es);
    quat_mul_pm(qn, en, qnp, qnm);
    quat_mul_pm(qs, es, qsp, qsm);
#pragma unroll
    for (int sgn = 0; sgn < 2; ++sgn) {
        const T (&a)[4] = sgn ? qnm : qnp;
        const T (&b)[4] = sgn ? qsm : qsp;
        T (&z)[7] = sgn ? zm : zp;
        const T sg = sgn ? T(-1) : T(1);
        const T rn = fast_rcp(fma(b[0], b[0], fma(b[1], b[1], fma(b[2], b[2], b[3] * b[3]))));
        const T qi[4] = {-b[0] * rn, -b[1] * rn, -b[2] * rn, b[3] * rn};   // q_s^-1, the quaternion taken as given
        const T d[3] = {fma(sg, dn[0] - ds[0], xn[0] - xs[0]), fma(sg, dn[1] - ds[1], xn[1] - xs[1]), fma(sg, dn[2] - ds[2], xn[2] - xs[2])};
        T r[3], dq[4];
        quat_rotate(qi, d, r);
        quat_mul(qi, a, dq);
        z[0] = r[0]; z[1] = r[1]; z[2] = r[2];
        z[3] = dq[0]; z[4] = dq[1]; z[5] = dq[2]; z[6] = dq[3];
    }
}

// z (-) ref on R^3 x SO(3), the parts a model does not read zeroed
template <class T> UKFB_DEV void relative_minus(const T (&z)[7], const T (&ref)[7], bool selp, bool selq, T (&d)[6]) {
    const T qz[4] = {z[3], z[4], z[5], z[6]}, qr[4] = {ref[3], ref[4], ref[5], ref[6]};
    T r[3];
    rot_minus(qz, qr, r);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        d[c] = selp ? (z[c] - ref[c]) : T(0);
        d[3 + c] = selq ? r[c] : T(0);
    }
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_relative_kernel(const RelativeArgs<T, TS> a) {
    static_assert(M::MODEL == 0, "relative measurements serve Pose engines");
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, NP = 4 * D + 1, PK = D * (D + 1) / 2;   // N: the chain's points, NP: the pairs
    constexpr RelativeMap LY = relative_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q, RT = MT<M>::RT;
    static_assert(Q == 3 && RT == 3, "position, then orientation: h reads the first six tangent rows");
    extern __shared__ __attribute__((aligned(16))) unsigned char delayed_smem[];
    uint32_t st = ST_OK;
    bool chain_ok = true;
    using ChainSample = RelativeSample<T, M, TS>;
#include "ukf_delayed_chain.inc.hpp"

    // ======================================================================= after the chain: the increment meets the pair (x_n, x_s)
    const DelayedRow<T, M, TS> row(a, delayed_smem, threadIdx.x);
    const auto& [l, lr, ls, fvalid, live, f, FAC, RSP, TAB, GM, MM, CSM, CSP, MUF, PKF, ROT, DUMP, SMR, MUP, MOP, Rn, Racc] = row;
    const RelativeSample<T, M, TS> smp(a, f, live);
    const bool selp = smp.selp, selq = smp.selq, do_u = smp.do_u;
    T* const NR = TAB + (LY.NR - LY.TAB);   // the rows of N = Sigma_n M^T
    T* const LE = SMR + (LY.LE - LY.SMR);   // the columns of L_e
    T* const PRK = SMR + (LY.PRK - LY.SMR);   // the parked scores (RELATIVE_PARK_*), once L_e is dead
    T* const WT = TAB + (LY.WT - LY.TAB);
    T* const YN = TAB + (LY.YN - LY.TAB);
    // the engine's present state into the (dead) filtered-record region
    MUF[l] = T(a.mu[f * S + ls]);
    for (int i = l; i < PK; i += 16) PKF[i] = T(a.cov[f * PK + i]);
    wsync();
    UKFB_MARK("r_cond");
    // ================================================================= 2a. Sigma_e = Sigma^s_s - M Sigma_n M^T: row lr
    T er[D];
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
#pragma unroll
        for (int c = 0; c < D; ++c) NR[lr * LS + c] = nr[c];
        wsync();
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            er[c] = CSP[hi * (hi + 1) / 2 + lo];
        }
#pragma nounroll
        for (int j = 0; j < D; ++j) {   // (M N)[lr][c] = sum_j M[lr][j] N[j][c]
            const T mj = MOP[lr * LS + j];
            const T* nrow = NR + j * LS;
#pragma unroll
            for (int c = 0; c < D; ++c) er[c] = fma(-mj, nrow[c], er[c]);
        }
    }
    wsync();
    UKFB_MARK("r_factors");
    // ================================================================= 2b. L_n = chol(Sigma_n) (scaled, in FAC), L_e clamped (in LE)
    bool ok1;
    {
        T arow[D];
        load_row<T, D>(PKF, l, arow);
        const T rs = chol16<T, D, LS>(arow, FAC, l, ok1);
        wsync();
        row_scale_factor<T, D, LS>(FAC, RSP, l, rs);
    }
    const bool oke = relative_chol_clamped<T, D, LS>(er, CSP[lr * (lr + 1) / 2 + lr], LE, l);
    wsync();
    UKFB_MARK("r_sigma");
    // ================================================================= 3. the 4 D + 1 pairs and Z = h(X_n, X_s)
    T z1p[7], z1m[7], z2p[7], z2m[7], ref[7];
    {
        T xn[7], xs[7], cn[6], cm[6], ce[6];
        const T zero6[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            xn[s] = MUF[s];
            xs[s] = CSM[s];
        }
        const T w = (l < D) ? T(1) : T(0);   // lanes >= D: the centre
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            cn[i] = FAC[lr * LS + i] * w;
            ce[i] = LE[lr * LS + i] * w;
            cm[i] = T(0);
        }
#pragma nounroll
        for (int k = 0; k < D; ++k) {   // rows 0 ... 5 of column lr of M L_n
            const T lk = FAC[lr * LS + k] * w;
#pragma unroll
            for (int i = 0; i < 6; ++i) cm[i] = fma(MOP[i * LS + k], lk, cm[i]);
        }
        sfence();
        relative_measure_pair(xn, xs, cn, cm, z1p, z1m);
        sfence();
        relative_measure_pair(xn, xs, zero6, ce, z2p, z2m);
#pragma unroll
        for (int c = 0; c < 7; ++c) ref[c] = row_bcast<D>(z1p[c]);
    }
    sfence();
    UKFB_MARK("r_mean");
    // ================================================================= 4a. z-bar: ukfom's iterated mean on R^3 x SO(3)
    const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
    bool conv = true;
    {
        bool active = do_u && chain_ok && ok1 && oke;
        int it = 0;
        while (wave_any(active)) {
            T dp[6];
            {
                T d[6];
                relative_minus(z1p, ref, selp, selq, d);
#pragma unroll
                for (int c = 0; c < 6; ++c) dp[c] = wp * d[c];
            }
            sfence();
            static_for<0, 3>([&](auto pc) {
                constexpr int p = decltype(pc)::value;
                T d[6];
                relative_minus(p == 0 ? z1m : (p == 1 ? z2p : z2m), ref, selp, selq, d);
#pragma unroll
                for (int c = 0; c < 6; ++c) dp[c] = fma(wm, d[c], dp[c]);
                sfence();
            });
            row_allreduce_n<T, 6>(dp);
            T m2 = T(0);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                dp[c] *= T(1) / T(NP);
                m2 = fma(dp[c], dp[c], m2);
            }
            const T dr[3] = {dp[3], dp[4], dp[5]}, qr[4] = {ref[3], ref[4], ref[5], ref[6]};
            T ex[4], nq[4];
            so3_exp_fast(dr, T(1), ex);
            quat_mul(qr, ex, nq);
#pragma unroll
            for (int c = 0; c < 3; ++c) ref[c] = active ? (ref[c] + dp[c]) : ref[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) ref[3 + c] = (active && selq) ? nq[c] : ref[3 + c];
            const bool more = m2 > a.mean_tol * a.mean_tol;
            const bool capped = more && (it + 1 >= a.mean_max_it);
            it += (active && more) ? 1 : 0;
            conv = conv && !(active && capped);
            active = active && more && !capped;
        }
    }
    UKFB_MARK("r_stats");
    // ================================================================= 4b. S = 1/2 sum dz dz^T + Q (identity outside the model's part), nu, W to LDS
    // (one point's delta at a time, in this order: the four of them at once do not fit the fp64 register file)
    T s21[21], nu[6];
    {
        const T hp = T(0.5) * wp, hm = T(0.5) * wm;
        T w[6];
        {
            T d[6];
            relative_minus(z1p, ref, selp, selq, d);
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                w[r] = d[r];
#pragma unroll
                for (int c = 0; c <= r; ++c) s21[r * (r + 1) / 2 + c] = (hp * d[r]) * d[c];
            }
        }
        sfence();
        {
            T d[6];
            relative_minus(z1m, ref, selp, selq, d);
            T* const dst = (l < D) ? (WT + l * ZS) : DUMP;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                dst[r] = wm * (T(0.5) * (w[r] - d[r]));
#pragma unroll
                for (int c = 0; c <= r; ++c) s21[r * (r + 1) / 2 + c] = fma(hm * d[r], d[c], s21[r * (r + 1) / 2 + c]);
            }
        }
        sfence();
        {
            T d[6];
            relative_minus(z2p, ref, selp, selq, d);
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) s21[r * (r + 1) / 2 + c] = fma(hm * d[r], d[c], s21[r * (r + 1) / 2 + c]);
        }
        sfence();
        {
            T d[6];
            relative_minus(z2m, ref, selp, selq, d);
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) s21[r * (r + 1) / 2 + c] = fma(hm * d[r], d[c], s21[r * (r + 1) / 2 + c]);
        }
        sfence();
        row_allreduce_n<T, 21>(s21);
        const TS* qp = a.Q + (a.q_uniform ? int64_t(0) : f * 36);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const bool used = ((r < 3) ? selp : selq) && ((c < 3) ? selp : selq);
                const T q = T(qp[6 * r + c]);
                s21[r * (r + 1) / 2 + c] = used ? (s21[r * (r + 1) / 2 + c] + q) : ((r == c) ? T(1) : T(0));
            }
        T zin[7];
        relative_load_sample<T, TS>(a, f, selp, selq, zin);
        relative_minus(zin, ref, selp, selq, nu);
    }
    wsync();
    UKFB_MARK("r_cross");
    // ================================================================= 4c. C_n row lr, S = Ls Ls^T in registers, Y_n = C_n Ls^-T, y = Ls^-1 nu
    // (the scores are parked for the stores at the end: L_e is dead, and the commit needs the registers)
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < 21; ++k) PRK[RELATIVE_PARK_S + k] = s21[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) PRK[RELATIVE_PARK_NU + k] = nu[k];
#pragma unroll
        for (int k = 0; k < 7; ++k) PRK[RELATIVE_PARK_ZBAR + k] = ref[k];
    }
    bool ok2;
    T d2, yn[6], yr[6];
    {
#pragma unroll
        for (int c = 0; c < 6; ++c) yr[c] = T(0);
#pragma nounroll
        for (int j = 0; j < D; ++j) {
            const T lj = FAC[j * LS + lr];
            const T* w = WT + j * ZS;
#pragma unroll
            for (int c = 0; c < 6; ++c) yr[c] = fma(lj, w[c], yr[c]);
        }
        T rs[6], lndet;
        relative_chol6(s21, rs, ok2, lndet);   // a pivot outside the model's part is exactly 1
        relative_solve6(yr, s21, rs);
#pragma unroll
        for (int c = 0; c < 6; ++c) yn[c] = nu[c];
        relative_solve6(yn, s21, rs);
        d2 = T(0);
#pragma unroll
        for (int c = 0; c < 6; ++c) d2 = fma(yn[c], yn[c], d2);
        T* const dst = (l < D) ? (YN + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 6; ++c) dst[c] = yr[c];
        if (l == 0) {
            PRK[RELATIVE_PARK_D2] = d2;
            PRK[RELATIVE_PARK_LNDET] = lndet;
        }
    }
    const bool accept = (a.gate_chi2 < T(0)) || (d2 <= a.gate_chi2);
    wsync();
    UKFB_MARK("r_cov_n");
    // ================================================================= 5. Sigma~_n = Sigma_n - Y_n Y_n^T: row lr, delta = Y_n y, the commit
    T sg[D], del[D];
    {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T* yc = YN + c * ZS;   // the rows other lanes wrote
            T v = PKF[hi * (hi + 1) / 2 + lo];
#pragma unroll
            for (int k = 0; k < 6; ++k) v = fma(-yr[k], yc[k], v);
            sg[c] = v;
        }
        T dl = T(0);
#pragma unroll
        for (int k = 0; k < 6; ++k) dl = fma(yr[k], yn[k], dl);
        static_for<0, D>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            del[c] = row_bcast<c>(dl);
        });
    }
    wsync();   // W, Y_n and the factors are dead
    UKFB_MARK("r_commit");
    T mnew[S];
    const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mnew);
    bool inf = false;
#pragma unroll
    for (int c = 0; c < D; ++c) inf = inf || !m_finite(sg[c]);
    const bool fin = !row_any(inf);
    const bool okc = chain_ok && ok1 && oke && ok2 && (!accept || (ok3 && fin));
    const bool good = do_u && okc && accept;
    st |= !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (smp.inactive ? ST_INACTIVE : (smp.old ? ST_ERR_NEG_DT : (smp.bad ? ST_ERR_NONFINITE_MEAS : ST_OK))));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && chain_ok && ok1 && oke && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && !accept) ? ST_REJECTED_GATE : 0u;

    UKFB_MARK("r_store");
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
        if (a.z_pred && l < 7) a.z_pred[f * 7 + l] = TS(scored ? (((l < 3) ? selp : selq) ? PRK[RELATIVE_PARK_ZBAR + l] : T(0)) : nanv);
        if (a.innov && l < 6) a.innov[f * 6 + l] = TS(scored ? PRK[RELATIVE_PARK_NU + l] : nanv);   // (zero outside the model's part)
        if (a.S)
            for (int e = l; e < 36; e += 16) {
                const int r = e / 6, c = e % 6, hi = r > c ? r : c, lo = r > c ? c : r;
                const bool used = ((r < 3) ? selp : selq) && ((c < 3) ? selp : selq);
                a.S[f * 36 + e] = TS(scored ? (used ? PRK[RELATIVE_PARK_S + hi * (hi + 1) / 2 + lo] : T(0)) : nanv);
            }
        if (l == 0) {
            const T m_ln2pi = T((selp ? 3 : 0) + (selq ? 3 : 0)) * T(1.8378770664093454835606594728112);
            const T d2p = PRK[RELATIVE_PARK_D2];
            if (a.maha) a.maha[f] = TS(scored ? d2p : nanv);
            if (a.loglik) a.loglik[f] = TS(scored ? T(-0.5) * (d2p + PRK[RELATIVE_PARK_LNDET] + m_ln2pi) : nanv);
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
}

}  // namespace ukfb
