// ukf_bearing.hpp -- bearing measurements: ukfom's update with the measurement manifold S^2.  h(X) = d(X) / |d(X)|, a unit vector
// in the sensor frame; the mean is iterated on the sphere, the differences are sphere logarithms, the noise is two-dimensional.
// Definitions: include/ukf_batch.h ("bearing measurements"), DESIGN.md 4.25.
//
// Layout and LDS map: the sensor-frame kernel's (ukf_sensor_meas.hpp: SensorArgs, sensor_map, sensor_solve3) on ukf_row.hpp --
// one filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup.
//  * lane l < D owns the sigma pair of factor column l and evaluates h on both points; lane D owns the centre.
//  * the sphere side lives in registers and in fp64 in every mode: the lane's two unit vectors, the reference of the mean
//    iteration, the logarithms.  A unit vector has entries of order one whatever the range to the landmark, so nothing is
//    gained by coordinates relative to Z_0 (the sensor-frame kernel's device); what fp32 could not carry is the tangent
//    vector t = v - (u.v) u of two directions a milliradian apart.
//  * the measurement side is three-dimensional and needs no tangent basis: with w_i = log_z-bar(Z_i) in the ambient frame,
//    Sigma_z = 1/2 sum w_i w_i^T and P Q P have z-bar in their null space, and S3 = Sigma_z + P Q P + c z-bar z-bar^T is block
//    diagonal in (any tangent basis, z-bar).  nu and the rows of C have no component along z-bar, so d^2 = nu^T S3^-1 nu and
//    K = C S3^-1 are the 2 x 2 quantities for every c > 0, and ln det S2 = ln det S3 - ln c.  The header's definition is c = 1;
//    the kernel takes c = trace(Sigma_z + P Q P) / 2, the mean tangent eigenvalue, so that S3 is as well conditioned as S2
//    (with c = 1 and Q of 1e-4 rad^2 the factorisation would lose four digits to the unit eigenvalue: all of fp32's margin).
//  * the three models differ by one per-row select (b - p or b) and a neutralised lever arm: one code path.
//  * a sigma point with |d|^2 zero or not finite is flagged where it arises and fails the row's S (ERR_CHOLESKY): the guarantee
//    does not lean on how NaN travels through the logarithms.
//  * a filter that fails, is gated, inactive or uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates (the mean iteration runs while any row is active; a converged row keeps its reference bit for bit).
//  * commit = 0: the kernel gets NULL for the state's output pointers -- it has nothing through which it could store.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// LDS per filter: sensor_map (ukf_host.hpp).
#pragma once

#include "ukf_row.hpp"
#include "ukf_sensor_meas.hpp"

namespace ukfb {

// What h reads beside the sigma point: the (neutralised) lever arm, the inverse of qs, the point, 1 / |q|^2 of the mean's
// orientation (every sigma point's orientation is the mean's times a unit exponential)
struct BearingIn {
    double r[3], qsi[4], b[3], rnq;
};

// d(X) / |d(X)| (include/ukf_batch.h); false: |d|^2 is zero or not finite
template <class M> UKFB_DEV bool bearing_h(const double (&x)[M::S], bool to_point, const BearingIn& in, double (&z)[3]) {
    constexpr int Q = MT<M>::Q;
    const double qi[4] = {-x[Q] * in.rnq, -x[Q + 1] * in.rnq, -x[Q + 2] * in.rnq, x[Q + 3] * in.rnq};
    double v[3] = {in.b[0], in.b[1], in.b[2]};
    if constexpr (M::MODEL == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = to_point ? (in.b[c] - x[c]) : in.b[c];   // b - p before anything is rotated
    }
    double g[3], o[3];
    quat_rotate(qi, v, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] -= in.r[c];   // (NAV_DIRECTION: r is neutral)
    quat_rotate(in.qsi, g, o);
    const double n2 = fma(o[0], o[0], fma(o[1], o[1], o[2] * o[2]));
    const double rn = fast_rsqrt(n2);
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = o[c] * rn;
    return pos_finite(n2);
}

// log_u(v) for unit u, v: theta t / |t|, t = v - (u.v) u, theta = atan2(|u x v|, u.v); exact zeros at v = u.  The result is
// tangent over the whole range, |u.w| <= 8 eps |w|.
//  * t is the tangent part of v - u (for unit u the same vector: u has none), projected against u twice.  v - u is zero to the
//    bit at v = u, and for directions a milliradian apart it is small and nearly exact, where v - fl(u.v) u is not: fl(u.v)
//    (and |u|^2 - 1) is off by an eps whatever |t| is, which stays in t as a RADIAL part.  One projection leaves such a part
//    towards the antipode as well, where |v - u| is 2 and u.(v - u) rounds at 3 eps: formed once, t gave w a radial share of
//    2e-4 at theta = 1e-12, 5e-8 at pi - 1e-8 and all of w at v = -u (fl(u.u) != 1: t = (fl(u.u) - 1) u != 0, the result
//    +-pi u).  The second projection takes it out to 2 eps of what it is given.
//  * Where |t| <= 4 eps is left with u.v < 0 the tangent part is not resolved: it is below the half ulp that each entry of v
//    carries, and the radial part the first projection left (<= 3 eps) is no longer small against it -- from 4 eps on the second
//    projection is given at most 1.75 |t| and leaves 3.5 eps |t|, inside the 8 eps above.  There, the exact antipode included, the
//    result is a tangent vector of length pi whose direction is unspecified (theta is within 4 eps of pi).
//  * theta = atan2(|t|, u.v): |u x v| = |t| for unit u (for |u|^2 = 1 + delta they differ by delta / 2, relative); |t| from the
//    reciprocal root k needs anyway and one Heron step, an ulp.  No cross product, no sqrt.
// NaN in, NaN out.
UKFB_DEV void s2_log(const double (&u)[3], const double (&v)[3], double (&w)[3]) {
    constexpr double UNRESOLVED2 = 0x1p-100;   // (4 eps)^2
    const double c = fma(u[0], v[0], fma(u[1], v[1], u[2] * v[2]));
    const double dv[3] = {v[0] - u[0], v[1] - u[1], v[2] - u[2]};
    const double e = fma(u[0], dv[0], fma(u[1], dv[1], u[2] * dv[2]));
    const double t0[3] = {fma(-e, u[0], dv[0]), fma(-e, u[1], dv[1]), fma(-e, u[2], dv[2])};
    const double d = fma(u[0], t0[0], fma(u[1], t0[1], u[2] * t0[2]));
    const double t[3] = {fma(-d, u[0], t0[0]), fma(-d, u[1], t0[1]), fma(-d, u[2], t0[2])};
    const double t2 = fma(t[0], t[0], fma(t[1], t[1], t[2] * t[2]));
    const double rt = fast_rsqrt(t2);
    const double s0 = t2 * rt;
    const double s = (t2 > 0.0) ? fma(0.5 * rt, fma(-s0, s0, t2), s0) : 0.0;   // |t|
    const double th = atan2(s, c);
    const double k = (t2 > 0.0) ? th * rt : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = k * t[i];   // (t = 0: zeros; t NaN: NaN)
    if (wave_any(t2 <= UNRESOLVED2 && c < 0.0)) {
        // e x u for the axis e in {e0, e1} farther from u: its norm is at least 0.6
        const bool first = m_abs(u[0]) < 0.6;
        const double p[3] = {first ? 0.0 : u[2], first ? -u[2] : 0.0, first ? u[1] : -u[0]};
        const double kp = 3.14159265358979323846 * fast_rsqrt(fma(p[0], p[0], fma(p[1], p[1], p[2] * p[2])));
        const bool anti = t2 <= UNRESOLVED2 && c < 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = anti ? kp * p[i] : w[i];
    }
}

// exp_u(w) = cos|w| u + sinc|w| w, renormalised
UKFB_DEV void s2_exp(const double (&u)[3], const double (&w)[3], double (&r)[3]) {
    double cs, sc;
    cos_sinc_sqrt(fma(w[0], w[0], fma(w[1], w[1], w[2] * w[2])), cs, sc);
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = fma(cs, u[i], sc * w[i]);
    const double rn = fast_rsqrt(fma(r[0], r[0], fma(r[1], r[1], r[2] * r[2])));
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] *= rn;
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_bearing_kernel(const SensorArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr SensorMap LY = sensor_map(S, D);
    constexpr int LS = LY.LS, ZS = LY.ZS, Q = MT<M>::Q;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(2 * D * ZS <= LY.MUF - LY.TAB && SENSOR_INPUT_SCALARS <= LY.DUM - LY.INP, "W, Y and the input record fit their regions");
    extern __shared__ __attribute__((aligned(16))) unsigned char bea_smem[];

    const RowCoords<M> rc(a.n, threadIdx.x);
    const int l = rc.l, lr = rc.lr, ls = rc.ls;
    const bool fvalid = rc.fvalid;
    const int64_t f = rc.f;
    T* const base = row_slice<T, LY.PF>(bea_smem, rc.g);
    T *const FAC = base + LY.FAC, *const RSP = base + LY.RSP, *const TAB = base + LY.TAB, *const WT = base + LY.WT;
    T *const YM = base + LY.YM, *const MUF = base + LY.MUF, *const PKF = base + LY.PKF, *const INP = base + LY.INP;
    T* const DUMP = base + LY.DUM;

    // ---- the row's filter, model and records
    const bool live = fvalid && a.initialised[f] != 0;
    const int mid = a.model ? a.model[f] : a.model_uniform;
    const bool mvalid = bearing_model_ok(M::MODEL, int64_t(mid));
    const int id = mvalid ? mid : (M::MODEL == 0 ? int(UKFB_BEARING_POSE_NAV_DIRECTION) : int(UKFB_BEARING_ORIENT_NAV_DIRECTION));   // no valid id: the row rides along
    row_stage_state<T, PK>(MUF, PKF, a.mu, a.cov, f * S, f * PK, l, ls);
    bool bad;
    {
        // the sensor-frame kernel's staging: lane i takes entries i and i + 16 of the record, judges its own and stores the
        // entry or, if the model does not read it, its neutral value
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
            const bool used = bearing_input_used(int64_t(id), i);
            b = b || (used && !m_finite(v));
            INP[i] = used ? v : T(sensor_input_neutral(i));
        }
        bad = row_any(b);
    }
    wsync();

    UKFB_MARK("n_sigma");
    // ================================================================= 1. sigma points of (mu, Sigma)
    T xp[S], xm[S];
    bool ok1;
    BearingIn hin;
    {
        T mu_r[S];
#pragma unroll
        for (int s = 0; s < S; ++s) mu_r[s] = MUF[s];
        {
            const double q0 = double(mu_r[Q]), q1 = double(mu_r[Q + 1]), q2 = double(mu_r[Q + 2]), q3 = double(mu_r[Q + 3]);
            hin.rnq = fast_rcp(fma(q0, q0, fma(q1, q1, fma(q2, q2, q3 * q3))));
        }
        ok1 = row_factorise<T, D, LS>(PKF, FAC, RSP, l);   // the scaled columns stay: C reads them
        T col[D];
        load_column<T, D, LS>(FAC, l, T(1), col);
        sigma_pair<T, M>(mu_r, col, xp, xm);               // lanes >= D: the centre twice (their column is zero)
    }
    sfence();
    UKFB_MARK("n_measure");
    // ================================================================= 2. Z = h(X) on the lane's pair, z^ = z / |z|: fp64 in every mode
    double zp[3], zm[3], zhat[3];
    bool degen;
    {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            hin.r[c] = double(INP[SENSOR_INPUT_MOUNT + c]);
            hin.b[c] = double(INP[SENSOR_INPUT_POINT + c]);
            zhat[c] = double(INP[SENSOR_INPUT_Z + c]);
        }
        {
            const double qs[4] = {double(INP[SENSOR_INPUT_MOUNT + 3]), double(INP[SENSOR_INPUT_MOUNT + 4]), double(INP[SENSOR_INPUT_MOUNT + 5]),
                                  double(INP[SENSOR_INPUT_MOUNT + 6])};
            const double rn = fast_rcp(fma(qs[0], qs[0], fma(qs[1], qs[1], fma(qs[2], qs[2], qs[3] * qs[3]))));
            hin.qsi[0] = -qs[0] * rn; hin.qsi[1] = -qs[1] * rn; hin.qsi[2] = -qs[2] * rn; hin.qsi[3] = qs[3] * rn;
        }
        {
            const double zz = fma(zhat[0], zhat[0], fma(zhat[1], zhat[1], zhat[2] * zhat[2]));   // (the same on every lane of the row)
            bad = bad || !pos_finite(zz);
            const double rn = fast_rsqrt(zz);
#pragma unroll
            for (int c = 0; c < 3; ++c) zhat[c] *= rn;
        }
        const bool to_point = id == UKFB_BEARING_POSE_POINT;
        using MH = typename M::template rebind<double>;
        double xh[S];
#pragma unroll
        for (int s = 0; s < S; ++s) xh[s] = double(xp[s]);
        const bool okp = bearing_h<MH>(xh, to_point, hin, zp);
        sfence();
#pragma unroll
        for (int s = 0; s < S; ++s) xh[s] = double(xm[s]);
        const bool okm = bearing_h<MH>(xh, to_point, hin, zm);
        sfence();
        degen = row_any(!(okp && okm));
    }
    const bool do_u = live && mvalid && !bad;
    sfence();
    UKFB_MARK("n_mean");
    // ================================================================= 3. z-bar: ukfom's iterated mean on S^2, from Z_0
    double ref[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ref[c] = row_bcast<D>(zp[c]);
    bool conv = true;
    const double wp = (l <= D) ? 1.0 : 0.0, wm = (l < D) ? 1.0 : 0.0;
    {
        const double tol2 = double(a.mean_tol) * double(a.mean_tol);
        bool active = do_u && ok1;
        int it = 0;
        while (wave_any(active)) {
            double lp[3], lm[3], dp[3], nref[3];
            s2_log(ref, zp, lp);
            s2_log(ref, zm, lm);
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = fma(wm, lm[c], wp * lp[c]);
            row_allreduce_n<double, 3>(dp);
            double m2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dp[c] *= 1.0 / double(N);
                m2 = fma(dp[c], dp[c], m2);
            }
            s2_exp(ref, dp, nref);
#pragma unroll
            for (int c = 0; c < 3; ++c) ref[c] = active ? nref[c] : ref[c];
            const bool more = m2 > tol2;   // (NaN: the row stops)
            const bool capped = more && (it + 1 >= a.mean_max_it);
            it += (active && more) ? 1 : 0;
            conv = conv && !(active && capped);
            active = active && more && !capped;
        }
    }
    UKFB_MARK("n_stats");
    // ================================================================= 4. Sigma_z = 1/2 sum w w^T, S = Sigma_z + P Q P, nu, W to LDS
    T s6[6], nu[3], zbar[3];
    T cz;   // the weight of z-bar z-bar^T in the factorised matrix
    {
        double lp[3], lm[3], ln[3];
        s2_log(ref, zp, lp);
        s2_log(ref, zm, lm);
        s2_log(ref, zhat, ln);
        T u[3], w[3];
        const double fu = (l == D) ? 0.70710678118654752440 : 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u[c] = T(wp * (fu * (0.5 * (lp[c] + lm[c]))));   // the centre's row: w_0 / sqrt 2; lanes beyond it: nothing
            w[c] = T(wm * (0.5 * (lp[c] - lm[c])));
            nu[c] = T(ln[c]);
            zbar[c] = T(ref[c]);
        }
        T* const dst = (l < D) ? (WT + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = w[c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) s6[r * (r + 1) / 2 + c] = fma(u[r], u[c], w[r] * w[c]);
        row_allreduce_n<T, 6>(s6);
        // P Q P = Q - z (Q z)^T - (Q z) z^T + (z^T Q z) z z^T, Q symmetric from its lower triangle
        double q6[6], qz[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) q6[r * (r + 1) / 2 + c] = double(INP[SENSOR_INPUT_Q + 3 * r + c]);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            qz[r] = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int hi = r > c ? r : c, lo = r > c ? c : r;
                qz[r] = fma(q6[hi * (hi + 1) / 2 + lo], ref[c], qz[r]);
            }
        }
        const double zqz = fma(ref[0], qz[0], fma(ref[1], qz[1], ref[2] * qz[2]));
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const double pqp = fma(zqz * ref[r], ref[c], fma(-qz[r], ref[c], fma(-ref[r], qz[c], q6[r * (r + 1) / 2 + c])));
                s6[r * (r + 1) / 2 + c] += T(pqp);
            }
        cz = T(0.5) * (s6[0] + s6[2] + s6[5]);
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
    UKFB_MARK("n_solve");
    // ================================================================= 6. S3 = S + cz z z^T = Ls Ls^T in registers; Y = C Ls^-T, y = Ls^-1 nu
    bool ok2;
    T lndet, d2, yn[3];
    {
        T s3[6];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) s3[r * (r + 1) / 2 + c] = fma(cz * zbar[r], zbar[c], s6[r * (r + 1) / 2 + c]);
        const T d0 = s3[0], i0 = fast_rcp(d0);
        const T t10 = s3[1] * i0, t20 = s3[3] * i0;
        const T d1 = fma(-t10, s3[1], s3[2]), a21 = fma(-t20, s3[1], s3[4]);
        const T i1 = fast_rcp(d1);
        const T d2p = fma(-(a21 * i1), a21, fma(-t20, s3[3], s3[5]));
        ok2 = (d0 > T(0)) && (d1 > T(0)) && (d2p > T(0)) && !degen;   // (NaN fails every comparison)
        lndet = m_log(d0) + m_log(d1) + m_log(d2p) - m_log(cz);     // ln det of the header's S3 (c = 1), of S2 in any basis
        const T rs[3] = {fast_rsqrt(d0), fast_rsqrt(d1), fast_rsqrt(d2p)};
        const T l10 = s3[1] * rs[0], l20 = s3[3] * rs[0], l21 = a21 * rs[1];
        sensor_solve3(cr, l10, l20, l21, rs);
#pragma unroll
        for (int c = 0; c < 3; ++c) yn[c] = nu[c];
        sensor_solve3(yn, l10, l20, l21, rs);
        d2 = fma(yn[0], yn[0], fma(yn[1], yn[1], yn[2] * yn[2]));
    }
    const bool accept = (a.gate_chi2 < T(0)) || (d2 <= a.gate_chi2);
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
    T mnew[S];
    const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mnew);
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
            if (a.z_pred) a.z_pred[f * 3 + l] = TS(scored ? zb : nanv);
            if (a.innov) a.innov[f * 3 + l] = TS(scored ? iv : nanv);
        }
        if (a.S && l < 9) {
            T v = T(0);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int r = k / 3, c = k % 3, hi = r > c ? r : c, lo = r > c ? c : r;
                v = (l == k) ? s6[hi * (hi + 1) / 2 + lo] : v;
            }
            a.S[f * 9 + l] = TS(scored ? v : nanv);
        }
        if (l == 0) {
            const T two_ln2pi = T(2.0 * 1.8378770664093454835606594728112);
            if (a.maha) a.maha[f] = TS(scored ? d2 : nanv);
            if (a.loglik) a.loglik[f] = TS(scored ? T(-0.5) * (d2 + lndet + two_ln2pi) : nanv);
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
}

}  // namespace ukfb
