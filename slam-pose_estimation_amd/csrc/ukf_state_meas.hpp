// ukf_state_meas.hpp -- joint state-block measurements: ukfom's update with z a sub-manifold of the state and h the selection of
// blocks, m up to D dimensions with a full covariance, per-filter block masks, covariance inflation (covariance intersection)
// and a read-only mode.  Definitions: include/ukf_batch.h ("joint state-block measurements"), DESIGN.md 4.16.
//
// Layout: the row layout (ukf_row.hpp) -- one filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup -- and
// its device functions: chol16 / load_column / sigma_pair, row_boxminus / row_boxplus, the D-column delta table, row-owned
// products and solves, row_factorise, the applyDelta commit (row_apply_delta).
//  * EVERY row works in all D dimensions whatever its mask: for an unselected dimension t column t of the table's deltas is zero,
//    row / column t of S is that of the identity and nu[t] = 0.  S is then blockdiag(S_sel, I) up to a permutation; the
//    subtractions of exact zeros leave the selected pivots' bits alone, column t of the solved cross-covariance is zero, and
//    d^2 and ln det S are those of the selection.  Four wave-mates with four masks take one code path.
//  * lane l < D owns the sigma pair of factor column l, row l of S, of C and of Sigma~; lane D owns the centre and, in the
//    solve, the innovation: y = Ls^-1 nu comes out of the same instructions that turn row l of C into row l of Y = C Ls^-T.
//    K S K^T = Y Y^T and K nu = Y y, so the second solve of K = C S^-1 is never made.
//  * a filter that fails, is gated, inactive or uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates (the mean iteration runs while any row is active; a converged row keeps its reference).
//  * commit = 0: the kernel gets NULL for the state's output pointers -- it has nothing through which it could store.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// LDS per filter: state_meas_map (ukf_host.hpp).
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

template <class T, class TS> struct StateMeasArgs {
    int64_t n;                   // filters
    const TS* mu;                // [n][S]
    const TS* cov;               // [n][PK]
    TS* mu_out;                  // the same arrays for commit = 1, null for commit = 0
    TS* cov_out;
    uint32_t* engine_status;     // [n]; null for commit = 0
    const uint8_t* initialised;  // [n]
    uint32_t mask_uniform;
    const int32_t* mask;         // [n] or null
    const TS* z;                 // [n][S]
    const TS* Qz;                // [n][PK]
    T infl_state, infl_meas;
    T mean_tol;
    int mean_max_it;
    T gate_chi2;                 // < 0: accept
    TS* maha;                    // [n] or null
    TS* loglik;                  // [n] or null
    uint32_t* status;            // [n] or null
};

// row_publish_deltas with the unselected columns zeroed (tsel: bit t = tangent dimension t is measured)
template <class T, class M, int LS>
UKFB_DEV void stm_publish_deltas(T* TAB, T* DUMP, int l, uint32_t tsel, const T (&xp)[M::S], const T (&xm)[M::S], const T (&ref)[M::S]) {
    constexpr int D = M::D;
    T dp[D], dm[D];
    row_boxminus<T, M>(xp, ref, dp);
    row_boxminus<T, M>(xm, ref, dm);
    T* const rowu = (l < D) ? (TAB + l * LS) : ((l == D) ? (TAB + 2 * D * LS) : DUMP);
    T* const roww = (l < D) ? (TAB + (D + l) * LS) : DUMP;
    const T fu = (l == D) ? T(0.70710678118654752440) : T(1);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const bool s = (tsel >> k) & 1u;
        rowu[k] = s ? fu * (T(0.5) * (dp[k] + dm[k])) : T(0);
        roww[k] = s ? T(0.5) * (dp[k] - dm[k]) : T(0);
    }
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_state_meas_kernel(const StateMeasArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr StateMeasMap LY = state_meas_map(S, D);   // the LDS slice (ukf_host.hpp)
    constexpr int LS = LY.LS, Q = MT<M>::Q, RT = MT<M>::RT, NB = (D + 2) / 3;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    static_assert(state_meas_blocks(M::MODEL) == NB, "tangent dimension t belongs to block t / 3");
    extern __shared__ __attribute__((aligned(16))) unsigned char stm_smem[];

    const RowCoords<M> rc(a.n, threadIdx.x);
    const int l = rc.l, lr = rc.lr, ls = rc.ls;
    const bool fvalid = rc.fvalid;
    const int64_t f = rc.f;
    T* const base = row_slice<T, LY.PF>(stm_smem, rc.g);
    T *const FAC = base + LY.FAC, *const RSP = base + LY.RSP, *const TAB = base + LY.TAB, *const YM = base + LY.YM;
    T *const MUF = base + LY.MUF, *const PKF = base + LY.PKF, *const ZM = base + LY.ZM, *const PKQ = base + LY.PKQ;
    T* const DUMP = base + LY.DUM;

    // ---- the row's filter, mask and records
    const bool live = fvalid && a.initialised[f] != 0;
    const int32_t mk = a.mask ? a.mask[f] : int32_t(a.mask_uniform);
    const bool mvalid = state_meas_mask_ok(NB, int64_t(mk));
    const uint32_t mbits = mvalid ? uint32_t(mk) : 0u;   // no valid mask: nothing is selected, the row rides along on the identity
    uint32_t tsel = 0u;
#pragma unroll
    for (int t = 0; t < D; ++t) tsel |= ((mbits >> (t / 3)) & 1u) << t;
    // (not row_stage_state: two records at once, the covariances inflated on the way)
    MUF[l] = T(a.mu[f * S + ls]);
    ZM[l] = T(a.z[f * S + ls]);
    for (int i = l; i < PK; i += 16) {
        PKF[i] = a.infl_state * T(a.cov[f * PK + i]);
        PKQ[i] = a.infl_meas * T(a.Qz[f * PK + i]);
    }
    wsync();
    // a SELECTED entry of z or Qz that is not finite: lane l looks at stored entry l of z and at row l of Qz
    bool bad;
    {
        const int tz = (ls < Q) ? ls : ((ls < Q + 4) ? RT : (ls - 1));   // a tangent dimension of stored entry ls's block
        bool b = ((tsel >> tz) & 1u) && !m_finite(ZM[ls]);
        const bool selr = (tsel >> lr) & 1u;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T q = PKQ[hi * (hi + 1) / 2 + lo];
            b = b || (selr && ((tsel >> c) & 1u) && !m_finite(q));
        }
        bad = row_any(b);
    }
    const bool do_u = live && mvalid && !bad;

    UKFB_MARK("m_sigma");
    // ================================================================= 1. sigma points of (mu, a Sigma)
    T xp[S], xm[S], ref[S];
    bool ok1;
    {
        T mu_r[S];
#pragma unroll
        for (int s = 0; s < S; ++s) mu_r[s] = MUF[s];
        ok1 = row_factorise<T, D, LS>(PKF, FAC, RSP, l);   // the scaled columns stay: C reads them
        T col[D];
        load_column<T, D, LS>(FAC, l, T(1), col);
        sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: the centre twice (their column is zero)
    }
    sfence();
#pragma unroll
    for (int s = 0; s < S; ++s) ref[s] = row_bcast<D>(xp[s]);   // Z_0 starts the mean
    UKFB_MARK("m_mean");
    // ================================================================= 2. z-bar: the iterated mean over the selected blocks
    bool conv = true;
    {
        const T wp = (l <= D) ? T(1) : T(0), wm = (l < D) ? T(1) : T(0);
        bool active = do_u && ok1;
        int it = 0;
        while (wave_any(active)) {
            T dp[D], dm[D];
            row_boxminus<T, M>(xp, ref, dp);
            row_boxminus<T, M>(xm, ref, dm);
#pragma unroll
            for (int c = 0; c < D; ++c) dp[c] = ((tsel >> c) & 1u) ? fma(wm, dm[c], wp * dp[c]) : T(0);
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
    UKFB_MARK("m_deltas");
    stm_publish_deltas<T, M, LS>(TAB, DUMP, l, tsel, xp, xm, ref);
    wsync();
    // ================================================================= 3. S = 1/2 sum dz dz^T + b Qz (identity outside the selection): row lr
    T srow[D];
    row_table_row<T, D, LS>(TAB, N, lr, srow);
    {
        const bool selr = (tsel >> lr) & 1u;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            const T q = PKQ[hi * (hi + 1) / 2 + lo];
            const bool both = selr && ((tsel >> c) & 1u);
            srow[c] = both ? (srow[c] + q) : ((c == lr) ? T(1) : T(0));
        }
    }
    sfence();
    // nu = z (-) z-bar over the selection (an unselected entry of z is never used: the reference's own takes its place)
    T nu[D];
    {
        T zf[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int tz = (s < Q) ? s : ((s < Q + 4) ? RT : (s - 1));
            const T zv = ZM[s];
            zf[s] = ((tsel >> tz) & 1u) ? zv : ref[s];
        }
        row_boxminus<T, M>(zf, ref, nu);
#pragma unroll
        for (int c = 0; c < D; ++c) nu[c] = ((tsel >> c) & 1u) ? nu[c] : T(0);
    }
    UKFB_MARK("m_cross");
    // ================================================================= 4. C = sum_j (L col j) W_j^T: row lr; lanes >= D carry nu instead
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
#pragma unroll
    for (int c = 0; c < D; ++c) cr[c] = (l < D) ? cr[c] : nu[c];
    wsync();   // the factor of a Sigma and the table are dead
    UKFB_MARK("m_solve");
    // ================================================================= 5. S = Ls Ls^T; Y = C Ls^-T row by row, y = Ls^-1 nu on lane D
    bool ok2;
    T lndet;
    {
        const T rs = chol16<T, D, LS>(srow, FAC, l, ok2);   // (not row_factorise_row: the unscaled pivots are read in between)
        wsync();
        const T pv = FAC[lr * LS + lr];   // the pivots, unscaled: det S is their product (an unselected one is exactly 1)
        lndet = row_allreduce((l < D) ? m_log(pv) : T(0));
        row_scale_factor<T, D, LS>(FAC, RSP, l, rs);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        T v = cr[k];
#pragma unroll
        for (int j = 0; j < k; ++j) v = fma(-FAC[j * LS + k], cr[j], v);
        cr[k] = v * RSP[k];
        sfence();
    }
    T yn[D];
    T d2 = T(0);
    static_for<0, D>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        yn[c] = row_bcast<D>(cr[c]);
        d2 = fma(yn[c], yn[c], d2);
    });
    const bool accept = (a.gate_chi2 < T(0)) || (d2 <= a.gate_chi2);
    {
        T* const dst = (l < D) ? (YM + l * LS) : DUMP;
#pragma unroll
        for (int c = 0; c < D; ++c) dst[c] = cr[c];
    }
    wsync();
    UKFB_MARK("m_cov");
    // ================================================================= 6. Sigma~ = a Sigma - Y Y^T: row lr, and delta = Y y
    T sg[D], del[D];
    {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            sg[c] = PKF[hi * (hi + 1) / 2 + lo];
        }
#pragma nounroll
        for (int j = 0; j < D; ++j) {
            const T yj = YM[lr * LS + j];
            const T* yc = YM + j;
#pragma unroll
            for (int c = 0; c < D; ++c) sg[c] = fma(-yj, yc[c * LS], sg[c]);   // the rows other lanes wrote
        }
        T dl = T(0);
#pragma unroll
        for (int c = 0; c < D; ++c) dl = fma(YM[lr * LS + c], yn[c], dl);
        static_for<0, D>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            del[c] = row_bcast<c>(dl);
        });
    }
    wsync();   // Y is dead
    UKFB_MARK("m_commit");
    // ================================================================= 7. commit: applyDelta(mu, Sigma~, delta)
    T mnew[S];
    const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mnew);
    const bool okc = ok1 && ok2 && (!accept || ok3);
    const bool good = do_u && okc && accept;
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!mvalid ? ST_INACTIVE : (bad ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (do_u && !okc) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && ok1 && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    st |= (do_u && okc && !accept) ? ST_REJECTED_GATE : 0u;

    UKFB_MARK("m_store");
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
    if (fvalid && l == 0) {
        const bool scored = do_u && okc;
        const T nanv = m_nan<T>();
        const T m_ln2pi = T(__builtin_popcount(tsel)) * T(1.8378770664093454835606594728112);
        if (a.maha) a.maha[f] = TS(scored ? d2 : nanv);
        if (a.loglik) a.loglik[f] = TS(scored ? T(-0.5) * (d2 + lndet + m_ln2pi) : nanv);
        if (a.status) a.status[f] = st;
        if (a.engine_status) a.engine_status[f] = st;
    }
}

}  // namespace ukfb
