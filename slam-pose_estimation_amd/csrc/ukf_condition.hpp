// ukf_condition.hpp -- covariance conditioning: eigenvalue repair of a filter's covariance in its correlation scaling, an optional
// renormalisation of the orientation quaternion; a read-only mode.  Definitions: include/ukf_batch.h ("covariance conditioning"),
// DESIGN.md 4.23.
//
// Layout: the tuned one (ukf_kernel16.hpp) -- one filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup.
//  * lane l < D owns row l of the working matrix M (C at the start) and row l of V (the identity at the start), register arrays
//    indexed by compile-time constants only; lanes >= D carry rows of zeros.
//  * cyclic Jacobi in a round-robin (tournament) ordering, the schedule a compile-time function of (step, pair): D = 12 plays
//    6 disjoint pairs in each of 11 steps; D = 13 is padded to 14 players with a decoupled unit row, 7 pairs in each of 13 steps,
//    and the pair of a step that holds the padding player is the identity (its m_pq is an exact zero, which the guard skips): it
//    is dropped at compile time, the padding row exists nowhere.  The only runtime loop is the sweep loop.
//  * a step: the three numbers of every pair (m_pp, m_qq, m_pq, all from lane p's row) are broadcast and kept by lanes p and q,
//    which compute the SAME (c, s) redundantly -- no branch, one division chain per lane and step instead of one per pair; the
//    column phase (M <- M J, V <- V J: every lane updates entries p and q of its two rows for every pair of the step, c and s
//    from row_bcast<p>); the row phase (M <- J^T M: every lane parks its row in the filter's LDS slice and combines it with its
//    partner's).
//  * convergence: one row all-reduction of the off-diagonal squares in front of every sweep, against (4 D u)^2.  A row that
//    passes publishes V and its diagonal to LDS THEN and is done: whatever its registers do in the sweeps its wave-mates still
//    need, nothing reads them again -- its bits cannot depend on its wave-mates.  The loop ends when every row is done or after
//    CONDITION_MAX_SWEEPS sweeps.
//  * the correction runs only when some row of the wavefront is deficient (wave-uniform): lane l forms row l of
//    sum_k w_k V[l][k] V[j][k] from the published V, adds its row of C (divided out of the packed covariance again, as at the
//    start) and writes s_l s_j C'_lj over ITS OWN packed row in LDS; a healthy row's packed record keeps the loaded bits.
//  * a filter that fails, is inactive or uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates.
//  * commit = 0: the kernel gets NULL for the state's output pointers -- it has nothing through which it could store.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// Global stores are plain vector stores.  LDS per filter: condition_map (ukf_host.hpp).
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

constexpr uint32_t ST_REPAIRED = 1u << 11;

template <class T, class TS> struct ConditionArgs {
    int64_t n;                   // filters
    const TS* mu;                // [n][S]
    const TS* cov;               // [n][PK]
    TS* mu_out;                  // the same arrays for commit = 1, null for commit = 0
    TS* cov_out;
    uint32_t* engine_status;     // [n]; null for commit = 0
    const uint8_t* initialised;  // [n]
    const TS* var_floor;         // [D]
    T eig_floor;                 // epsilon
    const uint8_t* select;       // [n] or null
    int renormalize;             // 0 / 1
    TS* eig_min;                 // [n] or null
    TS* eig_max;                 // [n] or null
    TS* mu_o;                    // [n][S] or null
    TS* cov_packed;              // [n][PK] or null
    uint32_t* status;            // [n] or null
};

template <class T> struct CondNum;
template <> struct CondNum<double> { static constexpr double u = 1.1102230246251565404e-16; };   // 2^-53
template <> struct CondNum<float> { static constexpr float u = 5.9604644775390625e-8f; };        // 2^-24

// The round-robin schedule (the circle method): DP = D rounded up to even players, player DP - 1 fixed, the others rotating; step
// r = 0 ... DP - 2 plays (DP - 1, r) and ((r + k) mod (DP - 1), (r - k) mod (DP - 1)), k = 1 ... DP / 2 - 1.  Every pair of
// players meets exactly once in a sweep, the pairs of a step are disjoint.  Where DP > D, player DP - 1 is the padding and
// pair k = 0 is dropped (condition_first_pair).
template <int D> struct CondSchedule {
    static constexpr int DP = condition_players(D), STEPS = DP - 1, K0 = condition_first_pair(D), KN = DP / 2;
    static constexpr int first(int r, int k) { return k == 0 ? DP - 1 : (r + k) % (DP - 1); }
    static constexpr int second(int r, int k) { return k == 0 ? r : (r - k + (DP - 1)) % (DP - 1); }
    static constexpr int p(int r, int k) { return first(r, k) < second(r, k) ? first(r, k) : second(r, k); }
    static constexpr int q(int r, int k) { return first(r, k) < second(r, k) ? second(r, k) : first(r, k); }
};

// One step r of a sweep on the rows of four filters.  guard: a pair with |m_pq| <= guard is not rotated (c = 1, s = 0).
template <int R, class T, int D, int LS> UKFB_DEV void cond_jacobi_step(T (&Mr)[D], T (&Vr)[D], T* ROWS, T* DUMP, int l, T guard) {
    using SC = CondSchedule<D>;
    // ---- the lane's pair: m_pp, m_qq, m_pq as lane p holds them (an idle lane: 1, 1, 0), its partner, its side
    T a = T(1), b = T(1), x = T(0);
    int pt = l;
    bool is_q = false;
    static_for<SC::K0, SC::KN>([&](auto kc) {
        constexpr int k = decltype(kc)::value, p = SC::p(R, k), q = SC::q(R, k);
        static_assert(p < q && q < D, "a pair of the schedule");
        const T mpp = row_bcast<p>(Mr[p]), mqq = row_bcast<q>(Mr[q]), mpq = row_bcast<p>(Mr[q]);
        const bool in = (l == p) || (l == q);
        a = in ? mpp : a;
        b = in ? mqq : b;
        x = in ? mpq : x;
        pt = (l == p) ? q : ((l == q) ? p : pt);
        is_q = is_q || (l == q);
    });
    // ---- (c, s) of the lane's pair, the same bits on lanes p and q
    T c, s;
    {
        const bool rot = m_abs(x) > guard;   // (NaN: no rotation)
        const T xs = rot ? x : T(1);
        const T th = (b - a) / (T(2) * xs);
        const T t = m_copysign(T(1), th) / (m_abs(th) + m_sqrt(fma(th, th, T(1))));
        const T cc = T(1) / m_sqrt(fma(t, t, T(1)));
        c = rot ? cc : T(1);
        s = rot ? t * cc : T(0);
    }
    // ---- column phase: entries p and q of the lane's rows of M and V, for every pair of the step
    static_for<SC::K0, SC::KN>([&](auto kc) {
        constexpr int k = decltype(kc)::value, p = SC::p(R, k), q = SC::q(R, k);
        const T cp = row_bcast<p>(c), sp = row_bcast<p>(s);
        const T mp = Mr[p], mq = Mr[q], vp = Vr[p], vq = Vr[q];
        Mr[p] = fma(-sp, mq, cp * mp);
        Mr[q] = fma(sp, mp, cp * mq);
        Vr[p] = fma(-sp, vq, cp * vp);
        Vr[q] = fma(sp, vp, cp * vq);
    });
    // ---- row phase: row p <- c row p - s row q, row q <- s row p + c row q, the partner's row through LDS
    {
        T* const wr = (l < D) ? (ROWS + l * LS) : DUMP;
#pragma unroll
        for (int j = 0; j < D; ++j) wr[j] = Mr[j];
        wsync();
        const T* const rd = ROWS + ((l < D) ? pt : 0) * LS;
        const T sl = is_q ? s : -s;
#pragma unroll
        for (int j = 0; j < D; ++j) Mr[j] = fma(sl, rd[j], c * Mr[j]);
        wsync();   // the rows are read: the next step may park its own
    }
}

// (the second bound: wavefronts per SIMD the register allocator must leave room for)
template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_condition_kernel(const ConditionArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2, Q = MT<M>::Q;
    constexpr ConditionMap LY = condition_map(S, D);   // the LDS slice (ukf_host.hpp)
    using SC = CondSchedule<D>;
    constexpr int LS = LY.LS;
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    extern __shared__ __attribute__((aligned(16))) unsigned char cnd_smem[];

    // (RowCoords' statements in place: built on it, this kernel left the spread of the parent's own runs -- profiles/row_toolkit_rates.txt)
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int lr = (l < D) ? l : (D - 1), ls = (l < S) ? l : (S - 1);
    const int64_t wg0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * ROW_FILTERS_PER_GROUP;
    const int64_t n_here = a.n - wg0;
    const int n_wg = int(n_here < ROW_FILTERS_PER_GROUP ? n_here : int64_t(ROW_FILTERS_PER_GROUP));
    const bool fvalid = g < n_wg;
    const int64_t f = wg0 + (fvalid ? g : (n_wg - 1));   // rows beyond the batch repeat its last filter and store nothing
    T* const base = reinterpret_cast<T*>(cnd_smem) + g * LY.PF;
    T *const ROWS = base + LY.ROW, *const VPB = base + LY.VPB, *const LAM = base + LY.LAM, *const SDV = base + LY.SDV;
    T *const MUF = base + LY.MUF, *const PKF = base + LY.PKF, *const DUMP = base + LY.DUM;

    // ---- the row's filter: the state to LDS, the lower triangle judged on the way; the floor judged where it lies
    const bool live = fvalid && a.initialised[f] != 0;
    const bool sel = !a.select || a.select[f] != 0;
    MUF[l] = T(a.mu[f * S + ls]);   // (not row_stage_state: the packed covariance is judged on the way)
    const T vfl = T(a.var_floor[lr]);
    bool nonfin, floor_bad;
    {
        bool b = false;
        for (int i = l; i < PK; i += 16) {
            const T v = T(a.cov[f * PK + i]);
            b = b || !m_finite(v);
            PKF[i] = v;
        }
        nonfin = row_any(b);
        floor_bad = row_any(!pos_finite(vfl));
    }
    wsync();
    UKFB_MARK("c_scale");
    // ---- d_t = max(Sigma_tt, v_t) as a comparison of stored numbers, s_t = sqrt(d_t); lanes >= D repeat lane D - 1
    const T dl_in = PKF[lr * (lr + 1) / 2 + lr];
    const bool raised_l = dl_in < vfl;
    const T d_l = raised_l ? vfl : dl_in, s_l = m_sqrt(d_l);
    SDV[lr] = s_l;
    const bool raised = row_any(raised_l);
    // ---- the quaternion of the mean, on every lane of the row
    T qrn = T(1);
    bool qbad = false, qmove = false;
    if (a.renormalize) {   // (wave-uniform)
        const T q0 = MUF[Q], q1 = MUF[Q + 1], q2 = MUF[Q + 2], q3 = MUF[Q + 3];
        const T qn2 = fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 * q0)));
        qrn = T(1) / m_sqrt(qn2);
        {
            qbad = !pos_finite(qn2);
            qmove = m_abs(qn2 - T(1)) > T(8) * T(CondNum<TS>::u);
        }
    }
    wsync();
    const bool fin = live && sel && !floor_bad && !nonfin && !qbad;

    // ---- C and the identity: row l
    T Mr[D], Vr[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const int hi = lr > j ? lr : j, lo = lr > j ? j : lr;
        const T cij = PKF[hi * (hi + 1) / 2 + lo] / (s_l * SDV[j]);
        Mr[j] = (l >= D) ? T(0) : ((l == j) ? T(1) : cij);
        Vr[j] = (l == j) ? T(1) : T(0);
    }
    // (a row that never passes the test leaves the identity behind: every LDS scalar the kernel reads is one it wrote)
    {
        T* const dv = (l < D) ? (VPB + l * LS) : DUMP;
#pragma unroll
        for (int k = 0; k < D; ++k) dv[k] = Vr[k];
        LAM[l] = T(1);
    }
    sfence();
    UKFB_MARK("c_jacobi");
    // ---- cyclic Jacobi; a row publishes V and its diagonal when it passes the test, and is done
    bool done = !fin, conv = false;
    {
        const T thr = T(4 * D) * CondNum<T>::u, thr2 = thr * thr, guard = CondNum<T>::u;
#pragma nounroll
        for (int sw = 0;; ++sw) {
            T off2 = T(0), dg = Mr[0];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const T t = (l == j || l >= D) ? T(0) : Mr[j];
                off2 = fma(t, t, off2);
                dg = (lr == j) ? Mr[j] : dg;
            }
            off2 = row_sum(off2);
            const bool newly = !done && (off2 <= thr2);   // (NaN fails the comparison)
            {
                const bool pub = newly && l < D;
                T* const dv = pub ? (VPB + l * LS) : DUMP;
#pragma unroll
                for (int k = 0; k < D; ++k) dv[k] = Vr[k];
                T* const de = pub ? (LAM + l) : (DUMP + 15);
                *de = dg;
            }
            conv = conv || newly;
            done = done || newly;
            if (sw == CONDITION_MAX_SWEEPS || !wave_any(!done)) break;
            static_for<0, SC::STEPS>([&](auto rc) { cond_jacobi_step<decltype(rc)::value, T, D, LS>(Mr, Vr, ROWS, DUMP, l, guard); });
        }
    }
    wsync();
    UKFB_MARK("c_verdict");
    const bool good = fin && conv;
    T emin, emax;
    {
        emin = LAM[good ? lr : 0];   // (a row that published nothing: whatever lies there, selected away below)
        emax = emin;
        emin = good ? emin : T(0);
        emax = good ? emax : T(0);
        row_minmax(emin, emax);
    }
    const bool fix = good && (raised || emin < T(0.5) * a.eig_floor);
    const bool rq = good && qmove;
    // ---- repair: C' = C + sum_{lambda_k < eps} (eps - lambda_k) v_k v_k^T, Sigma'_lj = s_l s_j C'_lj, the diagonal d_l C'_ll
    if (wave_any(fix)) {
        T u[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const T lam = LAM[k];
            const T w = (lam < a.eig_floor) ? (a.eig_floor - lam) : T(0);
            u[k] = w * VPB[lr * LS + k];
        }
        sfence();
#pragma nounroll
        for (int j = 0; j < D; ++j) {
            const T* const vj = VPB + j * LS;
            T acc = T(0);
#pragma unroll
            for (int k = 0; k < D; ++k) acc = fma(u[k], vj[k], acc);
            const int jj = j < lr ? j : lr;
            const int at = lr * (lr + 1) / 2 + jj;
            const T sj = SDV[j], ss = s_l * sj;
            const T cnew = (j == lr) ? (T(1) + acc) : (PKF[at] / ss + acc);
            const T snew = (j == lr) ? (d_l * cnew) : (ss * cnew);
            T* const dst = (fix && l < D && j <= l) ? (PKF + at) : DUMP;
            *dst = snew;
        }
    }
    wsync();
    UKFB_MARK("c_store");
    uint32_t st = !fvalid ? ST_OK : (!live ? ST_UNINITIALISED : (!sel ? ST_INACTIVE : (floor_bad ? ST_ERR_NONFINITE_MEAS : ST_OK)));
    st |= (live && sel && !floor_bad && !good) ? ST_ERR_CHOLESKY : 0u;
    st |= (fix || rq) ? ST_REPAIRED : 0u;
    const bool inq = l >= Q && l < Q + 4;
    const T mu_l = (rq && inq) ? (MUF[ls] * qrn) : MUF[ls];
    if (a.cov_out) {
        if (fix)
            for (int i = l; i < PK; i += 16) a.cov_out[f * PK + i] = TS(PKF[i]);
        if (rq && inq) a.mu_out[f * S + l] = TS(mu_l);
    }
    if (fvalid) {
        const T nanv = m_nan<T>();
        if (l < S && a.mu_o) a.mu_o[f * S + l] = TS(good ? mu_l : nanv);
        if (a.cov_packed)
            for (int i = l; i < PK; i += 16) a.cov_packed[f * PK + i] = TS(good ? PKF[i] : nanv);
        if (l == 0) {
            if (a.eig_min) a.eig_min[f] = TS(good ? emin : nanv);
            if (a.eig_max) a.eig_max[f] = TS(good ? emax : nanv);
            if (a.status) a.status[f] = st;
            if (a.engine_status) a.engine_status[f] = st;
        }
    }
}

}  // namespace ukfb
