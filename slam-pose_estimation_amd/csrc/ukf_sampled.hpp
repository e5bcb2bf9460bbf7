// ukf_sampled.hpp -- user-defined measurement models: the export of every filter's sigma points, and ukfom's update finished from
// the samples Z_i = h(X_i) the caller evaluated on them; measurement space R^m with m = 1 ... SAMPLED_MAX_M (one m for the
// launch), a read-only mode.  Definitions: include/ukf_batch.h ("user-defined measurement models"), DESIGN.md 4.21.
//
// Layout: the sensor-measurement kernel's (ukf_sensor_meas.hpp) -- one filter per 16-lane DPP row, four per wavefront, one
// wavefront per workgroup -- and the row toolkit's device functions (ukf_row.hpp): row_factorise, row_apply_delta.
// The update IS that kernel with Z_i = h(X_i) replaced by a load:
//  * the records in global memory are filter-major ([n][2 D + 1][...]): lane l < D owns the sigma pair of factor column l, rows
//    1 + 2 l and 2 + 2 l of its filter's record, adjacent, so that the export's lane writes 2 S contiguous scalars; lane D owns
//    the centre, row 0.  The update's row copies its filter's (2 D + 1) m contiguous samples into LDS with coalesced loads (and
//    judges them: ERR_NONFINITE_MEAS), then every lane takes its two.
//  * both kernels factorise Sigma with the same statements in the same order (load_row, chol16, row_scale_factor, load_column),
//    so that X_i (-) mu = +-L col j holds bit for bit for the points the caller evaluated; the update never reads X.
//  * the measurement side is SAMPLED_MAX_M-dimensional whatever m: m < 6 is embedded with zero deltas, identity rows / columns
//    of S and nu = 0 there (the argument of ukf_state_meas.hpp for unselected dimensions), so that every m takes one code path.
//  * S is 21 row all-reductions of u u^T + w w^T (u, w = half sum / half difference of the lane's two deltas; the centre adds
//    delta_0 delta_0^T / 2).  S goes to LDS for the outputs; its factor and y = Ls^-1 nu live in registers on every lane of the
//    row (sensor_solve3 extended to six).  Reductions, elimination steps and solves of dimensions beyond m are skipped by
//    wave-uniform branches (m is a kernel argument): they would add exact zeros and divide by exact ones.
//  * C row l = sum_j L[l][j] W_j^T: the factor columns and the D x 6 half differences from LDS with row-uniform reads; the row is
//    solved against Ls in registers (Y = C Ls^-T), and only the D x 6 matrix Y goes through LDS for Sigma~ = Sigma - Y Y^T.
//  * the differences Z_i - Z_0 and z - Z_0 are formed first, in fp64 in every mode, and the mean iteration, the deltas and the
//    innovation work on those differences (ukf_sensor_meas.hpp, for its reason): the update is invariant under a translation of
//    z and all Z_i together.
//  * a filter that fails, is gated, inactive or uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates (the mean iteration runs while any row is active; a converged row keeps its reference).
//  * commit = 0: the kernel gets NULL for the state's output pointers -- it has nothing through which it could store.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// LDS per filter: sampled_map, sigma_points_map (ukf_host.hpp).
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

template <class T, class TS> struct SigmaPointsArgs {
    int64_t n;                   // filters
    const TS* mu;                // [n][S]
    const TS* cov;               // [n][PK]
    const uint8_t* initialised;  // [n]
    TS* X;                       // [n][2 D + 1][S] or null
    TS* delta;                   // [n][2 D + 1][D] or null
    uint32_t* status;            // [n] or null
};

template <class T, class TS> struct SampledArgs {
    int64_t n;                   // filters
    const TS* mu;                // [n][S]
    const TS* cov;               // [n][PK]
    TS* mu_out;                  // the same arrays for commit = 1, null for commit = 0
    TS* cov_out;
    uint32_t* engine_status;     // [n]; null for commit = 0
    const uint8_t* initialised;  // [n]
    int m;                       // 1 ... SAMPLED_MAX_M
    const TS* Z;                 // [n][2 D + 1][m]
    const TS* z;                 // [n][m]
    const TS* Q;                 // [n][m][m], or [m][m] when q_uniform
    int q_uniform;
    const uint8_t* active;       // [n] or null
    T mean_tol;
    int mean_max_it;
    T gate_chi2;                 // < 0: accept
    TS* z_pred;                  // [n][m] or null
    TS* S;                       // [n][m][m] or null
    TS* innov;                   // [n][m] or null
    TS* maha;                    // [n] or null
    TS* loglik;                  // [n] or null
    uint32_t* status;            // [n] or null
};

// ---------------------------------------------------------------------------------------------------------------- the export
template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_sigma_points_kernel(const SigmaPointsArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr SigmaPointsMap LY = sigma_points_map(S, D);   // the LDS slice (ukf_host.hpp)
    constexpr int LS = LY.LS;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    extern __shared__ __attribute__((aligned(16))) unsigned char sgp_smem[];

    const RowCoords<M> rc(a.n, threadIdx.x);
    const int l = rc.l, ls = rc.ls;
    const bool fvalid = rc.fvalid;
    const int64_t f = rc.f;
    T* const base = row_slice<T, LY.PF>(sgp_smem, rc.g);
    T *const FAC = base + LY.FAC, *const RSP = base + LY.RSP, *const MUF = base + LY.MUF, *const PKF = base + LY.PKF;

    const bool live = fvalid && a.initialised[f] != 0;
    row_stage_state<T, PK>(MUF, PKF, a.mu, a.cov, f * S, f * PK, l, ls);
    wsync();
    // ---- the sigma points of (mu, Sigma): the statements of the update's step 1 (and of ukf_sensor_meas.hpp), in their order
    T xp[S], xm[S], mu_r[S], col[D];
    bool ok1;
    {
#pragma unroll
        for (int s = 0; s < S; ++s) mu_r[s] = MUF[s];
        ok1 = row_factorise<T, D, LS>(PKF, FAC, RSP, l);
        load_column<T, D, LS>(FAC, l, T(1), col);
        sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: their column is zero
    }
    sfence();
    // ---- lane l < D: rows 1 + 2 l and 2 + 2 l of the filter's record, adjacent; lane D: the centre, mu as it is stored
    if (fvalid) {
        const bool good = live && ok1;
        const T nanv = m_nan<T>();
        if (a.X) {
            TS* const rec = a.X + f * int64_t(N * S);
            if (l < D) {
                TS* const p = rec + (1 + 2 * l) * S;
#pragma unroll
                for (int s = 0; s < S; ++s) p[s] = TS(good ? xp[s] : nanv);
#pragma unroll
                for (int s = 0; s < S; ++s) p[S + s] = TS(good ? xm[s] : nanv);
            } else if (l == D) {
#pragma unroll
                for (int s = 0; s < S; ++s) rec[s] = TS(good ? mu_r[s] : nanv);
            }
        }
        if (a.delta) {
            TS* const rec = a.delta + f * int64_t(N * D);
            if (l < D) {
                TS* const p = rec + (1 + 2 * l) * D;
#pragma unroll
                for (int c = 0; c < D; ++c) p[c] = TS(good ? col[c] : nanv);
#pragma unroll
                for (int c = 0; c < D; ++c) p[D + c] = TS(good ? -col[c] : nanv);
            } else if (l == D) {
#pragma unroll
                for (int c = 0; c < D; ++c) rec[c] = TS(good ? T(0) : nanv);
            }
        }
        if (l == 0 && a.status) a.status[f] = !live ? ST_UNINITIALISED : (!ok1 ? ST_ERR_CHOLESKY : ST_OK);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the update
// c <- Ls^-1 c for the 6 x 6 factor held unscaled in the packed lower triangle lf (column k's entries are A[r][k] after step k
// of the elimination, so that Ls[r][k] = lf[r (r + 1) / 2 + k] * rs[k]) and the reciprocal roots of the pivots rs
// (m is wave-uniform: beyond it the factor is the identity and c is zero, the step would change nothing)
template <class T> UKFB_DEV void sampled_solve6(T (&c)[SAMPLED_MAX_M], const T (&lf)[21], const T (&rs)[SAMPLED_MAX_M], int m) {
#pragma unroll
    for (int k = 0; k < SAMPLED_MAX_M; ++k) {
        if (k < m) {
            T v = c[k];
#pragma unroll
            for (int j = 0; j < k; ++j) v = fma(-(lf[k * (k + 1) / 2 + j] * rs[j]), c[j], v);
            c[k] = v * rs[k];
        }
    }
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_sampled_kernel(const SampledArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr SampledMap LY = sampled_map(S, D);   // the LDS slice (ukf_host.hpp)
    constexpr int LS = LY.LS, ZS = LY.ZS, MM = LY.MM;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(LY.ZST - LY.TAB + N * MM <= LY.MUF - LY.TAB, "W, Y and the staged samples fit the table they alias");
    static_assert(SAMPLED_INPUT_SCALARS <= LY.DUM - LY.INP && MM * (MM + 1) / 2 == 21, "the input record fits its region");
    extern __shared__ __attribute__((aligned(16))) unsigned char smp_smem[];

    // (RowCoords' statements in place: built on it, this kernel left the spread of the parent's own runs -- profiles/row_toolkit_rates.txt)
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int lr = (l < D) ? l : (D - 1), ls = (l < S) ? l : (S - 1);
    const int64_t wg0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * ROW_FILTERS_PER_GROUP;
    const int64_t n_here = a.n - wg0;
    const int n_wg = int(n_here < ROW_FILTERS_PER_GROUP ? n_here : int64_t(ROW_FILTERS_PER_GROUP));
    const bool fvalid = g < n_wg;
    const int64_t f = wg0 + (fvalid ? g : (n_wg - 1));   // rows beyond the batch repeat its last filter and store nothing
    T* const base = reinterpret_cast<T*>(smp_smem) + g * LY.PF;
    T *const FAC = base + LY.FAC, *const RSP = base + LY.RSP, *const TAB = base + LY.TAB, *const WT = base + LY.WT;
    T *const YM = base + LY.YM, *const ZST = base + LY.ZST, *const MUF = base + LY.MUF, *const PKF = base + LY.PKF;
    T *const INP = base + LY.INP, *const DUMP = base + LY.DUM;
    const int m = a.m, mm = m * m;   // wave-uniform

    // ---- the row's filter and records: the state, z and Q (a lane takes entries l, l + 16, l + 32), the samples
    const bool live = fvalid && a.initialised[f] != 0;
    const bool act = !a.active || a.active[f] != 0;
    MUF[l] = T(a.mu[f * S + ls]);
    for (int i = l; i < PK; i += 16) PKF[i] = T(a.cov[f * PK + i]);
    bool bad;
    {
        bool b = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int i = l + 16 * p, j = i - SAMPLED_INPUT_Q;
            const bool is_z = i < m, is_q = j >= 0 && j < mm;
            int qr = 0;   // j / m
#pragma unroll
            for (int k = 1; k < MM; ++k) qr += (j >= k * m) ? 1 : 0;
            const bool lower = is_q && (j - qr * m) <= qr;
            const TS* src = a.z + f * m;   // (a safe address for the lanes that load nothing)
            src = is_z ? (a.z + f * m + i) : src;
            src = is_q ? (a.Q + (a.q_uniform ? int64_t(0) : f * mm) + j) : src;
            const T v = T(*src);
            b = b || ((is_z || lower) && !m_finite(v));
            if (i < SAMPLED_INPUT_S) INP[i] = (is_z || is_q) ? v : T(0);
        }
        const TS* zrec = a.Z + f * (int64_t(N) * m);
        for (int i = l; i < N * m; i += 16) {
            const T v = T(zrec[i]);
            b = b || !m_finite(v);
            ZST[i] = v;
        }
        bad = row_any(b);
    }
    wsync();
    const bool do_u = live && act && !bad;

    UKFB_MARK("u_sigma");
    // ================================================================= 1. L = chol(Sigma): the export's statements in their order
    bool ok1;
    {
        // (row_factorise's statements in place, in the export's order: called from here the fp32 instantiation left the spread
        // of the parent's own runs -- profiles/row_toolkit_rates.txt)
        T arow[D];
        load_row<T, D>(PKF, l, arow);
        const T rs = chol16<T, D, LS>(arow, FAC, l, ok1);
        wsync();
        row_scale_factor<T, D, LS>(FAC, RSP, l, rs);   // the scaled columns stay: C reads them
    }
    sfence();
    UKFB_MARK("u_measure");
    // ================================================================= 2. the lane's pair of samples, relative to Z_0
    // From here on the measurement side works in coordinates whose origin is Z_0 (ukf_sensor_meas.hpp): the differences are formed
    // in fp64 in every mode, before anything is rounded to the compute type.
    using TH = double;
    T zp[MM], zm[MM], zin[MM], ref[MM];
    TH z0[MM];
    {
        const int ip = ((l < D) ? (1 + 2 * l) : 0) * m, im = ((l < D) ? (2 + 2 * l) : 0) * m;
#pragma unroll
        for (int c = 0; c < MM; ++c) {
            const bool in_m = c < m;
            const int cc = in_m ? c : 0;   // (beyond m: an entry that exists, selected away)
            z0[c] = TH(ZST[cc]);           // Z_0 starts the mean
            const TH vp = TH(ZST[ip + cc]), vm = TH(ZST[im + cc]), vz = TH(INP[SAMPLED_INPUT_Z + cc]);
            zp[c] = in_m ? T(vp - z0[c]) : T(0);
            zm[c] = in_m ? T(vm - z0[c]) : T(0);
            zin[c] = in_m ? T(vz - z0[c]) : T(0);   // z - Z_0
            ref[c] = T(0);
        }
    }
    wsync();   // the staged samples are dead: W and Y may be written
    UKFB_MARK("u_mean");
    // ================================================================= 3. z-bar - Z_0: ukfom's iterated mean on R^6
    bool conv = true;
    const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
    {
        bool active = do_u && ok1;
        int it = 0;
        while (wave_any(active)) {
            T dp[MM];
#pragma unroll
            for (int c = 0; c < MM; ++c) dp[c] = fma(wm, zm[c] - ref[c], wp * (zp[c] - ref[c]));
#pragma unroll
            for (int c = 0; c < MM; ++c)
                if (c < m) dp[c] = row_sum(dp[c]);   // (beyond m every lane holds an exact zero: so is their sum)
            T m2 = T(0);
#pragma unroll
            for (int c = 0; c < MM; ++c) {
                dp[c] *= T(1) / T(N);
                m2 = fma(dp[c], dp[c], m2);
            }
#pragma unroll
            for (int c = 0; c < MM; ++c) ref[c] = active ? (ref[c] + dp[c]) : ref[c];
            const bool more = m2 > a.mean_tol * a.mean_tol;
            const bool capped = more && (it + 1 >= a.mean_max_it);
            it += (active && more) ? 1 : 0;
            conv = conv && !(active && capped);
            active = active && more && !capped;
        }
    }
    sfence();
    UKFB_MARK("u_stats");
    // ================================================================= 4. S = 1/2 sum dz dz^T + Q (identity beyond m), nu, W to LDS
    T s21[21], nu[MM];
    {
        T u[MM], w[MM];
        const T fu = (l == D) ? T(0.70710678118654752440) : T(1);
#pragma unroll
        for (int c = 0; c < MM; ++c) {
            const T dp = zp[c] - ref[c], dm = zm[c] - ref[c];
            u[c] = wp * (fu * (T(0.5) * (dp + dm)));      // the centre's row: delta_0 / sqrt 2; lanes beyond it: nothing
            w[c] = wm * (T(0.5) * (dp - dm));
        }
        T* const dst = (l < D) ? (WT + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < MM; ++c) dst[c] = w[c];
#pragma unroll
        for (int r = 0; r < MM; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) s21[r * (r + 1) / 2 + c] = fma(u[r], u[c], w[r] * w[c]);
#pragma unroll
        for (int r = 0; r < MM; ++r)
            if (r < m) {   // (wave-uniform; a row beyond m is replaced below)
#pragma unroll
                for (int c = 0; c <= r; ++c) s21[r * (r + 1) / 2 + c] = row_sum(s21[r * (r + 1) / 2 + c]);
            }
#pragma unroll
        for (int r = 0; r < MM; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const T q = INP[SAMPLED_INPUT_Q + ((r < m) ? (r * m + c) : 0)];
                s21[r * (r + 1) / 2 + c] = (r < m) ? (s21[r * (r + 1) / 2 + c] + q) : ((r == c) ? T(1) : T(0));   // (c <= r < m)
            }
        // S for the outputs: every lane of the row holds the same 21 values and stores them to the same addresses
#pragma unroll
        for (int r = 0; r < MM; ++r)
#pragma unroll
            for (int c = 0; c < MM; ++c) {
                const int hi = r > c ? r : c, lo = r > c ? c : r;
                INP[SAMPLED_INPUT_S + r * MM + c] = s21[hi * (hi + 1) / 2 + lo];
            }
        // so are z-bar and nu: parked for the outputs
#pragma unroll
        for (int c = 0; c < MM; ++c) {
            nu[c] = zin[c] - ref[c];
            INP[SAMPLED_INPUT_NU + c] = nu[c];
            INP[SAMPLED_INPUT_ZBAR + c] = T(z0[c] + TH(ref[c]));
        }
    }
    wsync();
    sfence();
    UKFB_MARK("u_cross");
    // ================================================================= 5. C = sum_j (L col j) W_j^T: row lr
    T cr[MM];
#pragma unroll
    for (int c = 0; c < MM; ++c) cr[c] = T(0);
#pragma nounroll
    for (int j = 0; j < D; ++j) {
        const T lj = FAC[j * LS + lr];
        const T* w = WT + j * ZS;
#pragma unroll
        for (int c = 0; c < MM; ++c) cr[c] = fma(lj, w[c], cr[c]);
    }
    sfence();
    UKFB_MARK("u_solve");
    // ================================================================= 6. S = Ls Ls^T in registers; Y = C Ls^-T, y = Ls^-1 nu
    bool ok2 = true;
    T lndet = T(0), d2 = T(0), yn[MM];
    {
        T rs[MM];
#pragma unroll
        for (int k = 0; k < MM; ++k) {
            rs[k] = T(1);
            if (k < m) {   // (wave-uniform) a pivot beyond m is exactly 1 and heads a column of zeros: its step changes nothing
                const T dk = s21[k * (k + 1) / 2 + k], ik = fast_rcp(dk);
                ok2 = ok2 && (dk > T(0));   // (NaN fails every comparison)
                lndet += m_log(dk);
                rs[k] = fast_rsqrt(dk);
#pragma unroll
                for (int r = k + 1; r < MM; ++r) {
                    if (r < m) {
                        const T t = s21[r * (r + 1) / 2 + k] * ik;
#pragma unroll
                        for (int c = k + 1; c <= r; ++c) s21[r * (r + 1) / 2 + c] = fma(-t, s21[c * (c + 1) / 2 + k], s21[r * (r + 1) / 2 + c]);
                    }
                }
            }
        }
        sfence();
        sampled_solve6(cr, s21, rs, m);
#pragma unroll
        for (int c = 0; c < MM; ++c) yn[c] = nu[c];
        sampled_solve6(yn, s21, rs, m);
        sfence();
#pragma unroll
        for (int c = 0; c < MM; ++c) d2 = fma(yn[c], yn[c], d2);
    }
    const bool accept = (a.gate_chi2 < T(0)) || (d2 <= a.gate_chi2);
    {
        T* const dst = (l < D) ? (YM + l * ZS) : DUMP;
#pragma unroll
        for (int c = 0; c < MM; ++c) dst[c] = cr[c];
    }
    wsync();
    sfence();
    UKFB_MARK("u_cov");
    // ================================================================= 7. Sigma~ = Sigma - Y Y^T: row lr, and delta = Y y
    T sg[D], del[D];
    {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T* yc = YM + c * ZS;   // the rows other lanes wrote
            T v = PKF[hi * (hi + 1) / 2 + lo];
#pragma unroll
            for (int k = 0; k < MM; ++k) v = fma(-cr[k], yc[k], v);
            sg[c] = v;
        }
        T dl = T(0);
#pragma unroll
        for (int k = 0; k < MM; ++k) dl = fma(cr[k], yn[k], dl);
        static_for<0, D>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            del[c] = row_bcast<c>(dl);
        });
    }
    wsync();   // W, Y and the factor of Sigma are dead
    sfence();
    UKFB_MARK("u_commit");
    // ================================================================= 8. commit: applyDelta(mu, Sigma~, delta)
    T mnew[S];
    const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mnew);
    const bool okc = ok1 && ok2 && (!accept || ok3);
    const bool good = do_u && okc && accept;
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!act ? ST_INACTIVE : (bad ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && ok1 && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && !accept) ? ST_REJECTED_GATE : 0u;

    UKFB_MARK("u_store");
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
        {
            const int lm = (l < m) ? l : 0;
            const T zb = INP[SAMPLED_INPUT_ZBAR + lm], iv = INP[SAMPLED_INPUT_NU + lm];
            if (l < m && a.z_pred) a.z_pred[f * m + l] = TS(scored ? zb : nanv);
            if (l < m && a.innov) a.innov[f * m + l] = TS(scored ? iv : nanv);
        }
        if (a.S) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const int k = l + 16 * p;
                int r = 0;   // k / m
#pragma unroll
                for (int q = 1; q < MM; ++q) r += (k >= q * m) ? 1 : 0;
                const T v = INP[SAMPLED_INPUT_S + ((k < mm) ? (r * MM + (k - r * m)) : 0)];
                if (k < mm) a.S[f * mm + k] = TS(scored ? v : nanv);
            }
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
