// ukf_row.hpp -- the device toolkit of the row layout the feature kernels share with the tuned kernel (ukf_kernel16.hpp): one
// filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup, every filter with its own slice of the
// workgroup's LDS.  What is here:
//  * neutral helpers: row reductions (row_any, row_sum, row_minmax), m_nan / m_log / m_exp / m_min / m_max / m_copysign;
//  * the manifold helpers of the sigma-point kernels: row_boxminus / row_boxplus (the fast SO(3) maps of the forward kernel), the
//    delta table (row_publish_deltas, row_table_row), the scaled factor (row_scale_factor);
//  * the blocks every feature kernel is made of: RowCoords (what a lane derives from its index), row_stage_state (a record into
//    LDS), row_factorise (Sigma = L L^T, scaled, with its reciprocal pivots), row_apply_delta (ukfom's applyDelta: the commit of
//    every update).
// A feature header includes this file, and a sibling feature only where it calls that feature's own device functions
// (DESIGN.md 4.24).  Everything is forced inline; the statements are those of the kernels they came from, in their order.
// UKFB_MARK stays in the kernel bodies: it names the kernel's argument and counts with __COUNTER__.
#pragma once

#include "ukf_kernel16.hpp"
#include "ukf_host.hpp"

namespace ukfb {

// the second launch bound of the row kernels: wavefronts per SIMD the register allocator must leave room for (the LDS slices
// admit no more in fp64)
constexpr int ROW_WAVES_PER_SIMD = 2;

// ---------------------------------------------------------------------------------------------------------------- neutral helpers
UKFB_DEV double m_log(double x) { return log(x); }
UKFB_DEV float m_log(float x) { return logf(x); }
UKFB_DEV double m_exp(double x) { return exp(x); }
UKFB_DEV float m_exp(float x) { return expf(x); }
UKFB_DEV double m_copysign(double m, double s) { return __builtin_copysign(m, s); }
UKFB_DEV float m_copysign(float m, float s) { return __builtin_copysignf(m, s); }
UKFB_DEV double m_min(double a, double b) { return __builtin_fmin(a, b); }
UKFB_DEV float m_min(float a, float b) { return __builtin_fminf(a, b); }
UKFB_DEV double m_max(double a, double b) { return __builtin_fmax(a, b); }
UKFB_DEV float m_max(float a, float b) { return __builtin_fmaxf(a, b); }
template <class T> UKFB_DEV T m_nan() { return T(__builtin_nanf("")); }

// the row's OR of a per-lane flag
UKFB_DEV bool row_any(bool b) { return row_allreduce(b ? 1.0f : 0.0f) != 0.0f; }
// one row all-reduction (the butterflies need all 64 lanes: callers branch on wave-uniform conditions only)
template <class T> UKFB_DEV T row_sum(T v) {
    T one[1] = {v};
    row_allreduce_n<T, 1>(one);
    return one[0];
}
// min / max over a 16-lane row, the butterflies of row_allreduce(float): every lane of the row ends with the same bits
template <class T> UKFB_DEV void row_minmax(T& lo, T& hi) {
    lo = m_min(lo, dpp_mov<0xB1>(lo));
    hi = m_max(hi, dpp_mov<0xB1>(hi));
    lo = m_min(lo, dpp_mov<0x4E>(lo));
    hi = m_max(hi, dpp_mov<0x4E>(hi));
    lo = m_min(lo, dpp_mov<0x141>(lo));
    hi = m_max(hi, dpp_mov<0x141>(hi));
    lo = m_min(lo, dpp_mov<0x140>(lo));
    hi = m_max(hi, dpp_mov<0x140>(hi));
}

// ---------------------------------------------------------------------------------------------------------------- manifold helpers
// x (-) y and x (+) d with the fast SO(3) maps of the forward kernel
template <class T, class M> UKFB_DEV void row_boxminus(const T (&x)[M::S], const T (&y)[M::S], T (&d)[M::D]) {
    constexpr int Q = MT<M>::Q, RT = MT<M>::RT, D = M::D;
#pragma unroll
    for (int t = 0; t < D; ++t) {
        if (t < RT) d[t] = x[t] - y[t];
        else if (t >= RT + 3) d[t] = x[t + 1] - y[t + 1];
    }
    const T qx[4] = {x[Q], x[Q + 1], x[Q + 2], x[Q + 3]}, qy[4] = {y[Q], y[Q + 1], y[Q + 2], y[Q + 3]};
    T r[3];
    rot_minus(qx, qy, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[RT + k] = r[k];
}
template <class T, class M> UKFB_DEV void row_boxplus(const T (&x)[M::S], const T (&d)[M::D], T (&o)[M::S]) {
    constexpr int Q = MT<M>::Q, RT = MT<M>::RT, D = M::D;
#pragma unroll
    for (int t = 0; t < D; ++t) {
        if (t < RT) o[t] = x[t] + d[t];
        else if (t >= RT + 3) o[t + 1] = x[t + 1] + d[t];
    }
    const T q[4] = {x[Q], x[Q + 1], x[Q + 2], x[Q + 3]};
    const T v[3] = {d[RT], d[RT + 1], d[RT + 2]};
    T e[4], r[4];
    so3_exp_fast(v, T(1), e);
    quat_mul(q, e, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[Q + k] = r[k];
}

// Deltas of the lane's sigma pair to `ref` into the table: row l = U_l, row D + l = W_l, the centre lane's row 2 D = delta_0 / sqrt 2
// (half sums and half differences: 1/2 sum d d^T = sum over the rows of row row^T)
template <class T, class M, int LS>
UKFB_DEV void row_publish_deltas(T* TAB, T* DUMP, int l, const T (&xp)[M::S], const T (&xm)[M::S], const T (&ref)[M::S]) {
    constexpr int D = M::D;
    T dp[D], dm[D];
    row_boxminus<T, M>(xp, ref, dp);
    row_boxminus<T, M>(xm, ref, dm);
    T* const rowu = (l < D) ? (TAB + l * LS) : ((l == D) ? (TAB + 2 * D * LS) : DUMP);
    T* const roww = (l < D) ? (TAB + (D + l) * LS) : DUMP;
    const T fu = (l == D) ? T(0.70710678118654752440) : T(1);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        rowu[k] = fu * (T(0.5) * (dp[k] + dm[k]));
        roww[k] = T(0.5) * (dp[k] - dm[k]);
    }
}

// row lr of sum_{i < rows} TAB_i TAB_i^T (all D columns; the same bits at (r, c) and (c, r))
template <class T, int D, int LS> UKFB_DEV void row_table_row(const T* TAB, int rows, int lr, T (&out)[D]) {
#pragma unroll
    for (int c = 0; c < D; ++c) out[c] = T(0);
#pragma nounroll
    for (int i = 0; i < rows; ++i) {
        const T* r = TAB + i * LS;
        const T own = r[lr];
#pragma unroll
        for (int c = 0; c < D; ++c) out[c] = fma(own, r[c], out[c]);
    }
}

// scaled factor in place of chol16's unscaled columns (zeros above the diagonal), reciprocal pivots behind it
template <class T, int D, int LS> UKFB_DEV void row_scale_factor(T* FAC, T* RSP, int l, T rs) {
    T col[D];
    load_column<T, D, LS>(FAC, l, rs, col);
    wsync();
    T* dst = FAC + ((l < D) ? l : (D - 1)) * LS;
    if (l < D) {
#pragma unroll
        for (int c = 0; c < D; ++c) dst[c] = col[c];
        RSP[l] = rs;
    }
    wsync();
}

// ---------------------------------------------------------------------------------------------------------------- the blocks
// What a lane derives from its index: its row g of the wavefront and its lane l of the row, l clamped to a row of the matrices
// (lr) and to an entry of the mean (ls), and the row's filter of a batch of n
template <class M> struct RowCoords {
    int l, lr, ls, g;
    bool fvalid;   // the row has a filter of the batch
    int64_t f;     // rows beyond the batch repeat its last filter and store nothing
    UKFB_DEV RowCoords(int64_t n, int lane) {
        g = lane >> 4;
        l = lane & 15;
        lr = (l < M::D) ? l : (M::D - 1);
        ls = (l < M::S) ? l : (M::S - 1);
        const int64_t wg0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * ROW_FILTERS_PER_GROUP;
        const int64_t n_here = n - wg0;
        const int n_wg = int(n_here < ROW_FILTERS_PER_GROUP ? n_here : int64_t(ROW_FILTERS_PER_GROUP));
        fvalid = g < n_wg;
        f = wg0 + (fvalid ? g : (n_wg - 1));
    }
};
// the LDS slice of row g: PF scalars of the compute type per filter
template <class T, int PF> UKFB_DEV T* row_slice(unsigned char* smem, int g) { return reinterpret_cast<T*>(smem) + g * PF; }

// a record of the arrays mu and cov, at scalar offsets mean_at / pack_at, into MEAN (16) and PACK in the compute type.  The
// offsets are the caller's expressions (f * S, f * PK): it forms them again for its stores, and the compiler shares them.
template <class T, int PK, class TS> UKFB_DEV void row_stage_state(T* MEAN, T* PACK, const TS* mu, const TS* cov, int64_t mean_at, int64_t pack_at, int l, int ls) {
    MEAN[l] = T(mu[mean_at + ls]);
    for (int i = l; i < PK; i += 16) PACK[i] = T(cov[pack_at + i]);
}

// the lane's row `arow` of a symmetric matrix -> its scaled factor in FAC, the reciprocal pivots in RSP; returns chol16's verdict
template <class T, int D, int LS> UKFB_DEV bool row_factorise_row(T (&arow)[D], T* FAC, T* RSP, int l) {
    bool ok;
    const T rs = chol16<T, D, LS>(arow, FAC, l, ok);
    wsync();
    row_scale_factor<T, D, LS>(FAC, RSP, l, rs);
    return ok;
}
// the same of the packed matrix PACK: the export's statements in their order, so that the sigma points X_i (-) mu = +-L col j
// agree bit for bit between the export and the kernels that finish from samples.  ukf_sampled_kernel, ukf_sensor_meas_kernel and
// ukf_delayed_kernel keep these statements in place (their own comments say why): a change here is repeated there.
template <class T, int D, int LS> UKFB_DEV bool row_factorise(const T* PACK, T* FAC, T* RSP, int l) {
    T arow[D];
    load_row<T, D>(PACK, l, arow);
    return row_factorise_row<T, D, LS>(arow, FAC, RSP, l);
}

// commit: applyDelta(mu, Sigma~, delta) -- factorise Sigma~ (the lane's row in sg), re-sample around mu [+] delta, deltas against
// that point.  mu is read from MEAN into mu_r; on return mnew = mu [+] delta and sg is the lane's row of the re-sampled
// covariance (the centre's row of the table: exact zeros but for log(conj(q) q)).  Returns the verdict on Sigma~.
// ukf_sensor_meas_kernel and ukf_delayed_kernel (twice) keep these statements in place: a change here is repeated there.
template <class T, class M, int LS>
UKFB_DEV bool row_apply_delta(T* FAC, T* TAB, const T* MEAN, T* DUMP, int l, int lr, const T (&del)[M::D], T (&sg)[M::D], T (&mu_r)[M::S],
                              T (&mnew)[M::S]) {
    constexpr int S = M::S, D = M::D;
    bool ok3;
    {
        const T rs = chol16<T, D, LS>(sg, FAC, l, ok3);
        wsync();
        T col[D], dpl[D], dmi[D], xp[S], xm[S];
        load_column<T, D, LS>(FAC, l, rs, col);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            dpl[c] = del[c] + col[c];
            dmi[c] = del[c] - col[c];
        }
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) mu_r[s2] = MEAN[s2];   // (reloaded: not kept live across the kernel)
        sfence();
        row_boxplus<T, M>(mu_r, del, mnew);
        row_boxplus<T, M>(mu_r, dpl, xp);
        row_boxplus<T, M>(mu_r, dmi, xm);
        row_publish_deltas<T, M, LS>(TAB, DUMP, l, xp, xm, mnew);
    }
    wsync();
    row_table_row<T, D, LS>(TAB, 2 * D, lr, sg);
    return ok3;
}
template <class T, class M, int LS>
UKFB_DEV bool row_apply_delta(T* FAC, T* TAB, const T* MEAN, T* DUMP, int l, int lr, const T (&del)[M::D], T (&sg)[M::D], T (&mnew)[M::S]) {
    T mu_r[M::S];
    return row_apply_delta<T, M, LS>(FAC, TAB, MEAN, DUMP, l, lr, del, sg, mu_r, mnew);
}

}  // namespace ukfb
