// ukf_smooth.hpp -- fixed-interval smoothing on the device: the manifold Rauch-Tung-Striebel backward pass over a window of
// filtered states that the caller recorded in device rings (ukfb_history_push_dev).  READ-ONLY on the engine: the kernel has no
// pointer to the engine's state through which it could store.  Definitions: include/ukf_batch.h ("fixed-interval smoothing"),
// DESIGN.md 4.15.
//
// Layout: the tuned one (ukf_kernel16.hpp) -- one filter per 16-lane DPP row, four per wavefront, one wavefront per workgroup.
//  * chain residency: the smoothed state of the step above (mean, packed covariance) stays in LDS in the compute type between
//    the steps of a launch; per step only the filtered record comes in from HBM and only the smoothed record leaves.
//  * the prediction is REDONE from the filtered record with the forward kernel's device functions in its order (chol16,
//    load_column, sigma_pair, process_fast, the iterated mean, process_noise_entry16): lane l < D owns the sigma pair of factor
//    column l, lane D the centre.  The sigma-point deltas go to a table in LDS as half sums U_l and half differences W_l
//    (1/2 sum d d^T = sum over the rows of row row^T, as Layout16's table); unlike the forward kernel the table has all D
//    columns, because the cross-covariance needs every component.
//  * lane l < D owns row l of Sigma^-, C, G, the transported Sigma^t, M = Sigma^t - Sigma^- and Sigma~.  Row x matrix products
//    and the two triangular solves read the shared operand (the table, the factor of Sigma^-, M, G) from LDS at an address
//    that is the same for the whole row: a broadcast, no bank conflicts.  C takes the factor columns directly
//    (X_j+- (-) mu = +-L col j): C = sum_j L col j W_j^T.
//  * transport: Jr^-1(phi) on the SO(3) block, the congruence of ukf_bank.hpp (three-column product inside the lane, three-row
//    product over the rotation's lanes).
//  * commit: applyDelta(mu, Sigma~, G e) -- factorise Sigma~, re-sample around mu [+] G e, deltas against that point.
//  * a filter that fails, is gated or is uninitialised rides along: every select is per row, no row's bits depend on its
//    wave-mates (the mean iteration runs while any row is active; a converged row keeps its reference).
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// LDS per filter: smooth_map (ukf_host.hpp) -- the factor region (Sigma's, then Sigma^-'s, then Sigma~'s), the delta
// table (aliased by G and M once C and Sigma^- are formed), the chain record, the filtered record, the rotation matrix, a sink.
#pragma once

#include "ukf_row.hpp"
#include "ukf_bank.hpp"   // bank_jrinv_coeff

namespace ukfb {

template <class T, class TS> struct SmoothArgs {
    int64_t n;                   // filters
    const TS* mu_hist;           // [slots][n][S]
    const TS* cov_hist;          // [slots][n][PK]
    TS* mu_out;                  // [slots][n][S]
    TS* cov_out;                 // [slots][n][PK] or null
    const TS* start_mu;          // [n][S]   the chain's state above the first backward step of this launch
    const TS* start_cov;         // [n][PK]
    TS* end_cov;                 // [n][PK] or null: receives the chain covariance after the last step (cov_out == null, more launches follow)
    int copy_top;                // bit 0 / 1: store the start record's mean / covariance to slot top_slot of the outputs
    int slots, top_slot, back;   // ring size, slot of the start record's step, backward steps of this launch (<= SMOOTH_MAX_BACK)
    const uint8_t* initialised;  // [n]
    const TS* Rn;                // process noise, D * D row-major; per filter if Rn_stride != 0
    int64_t Rn_stride;
    const TS* Racc;              // Pose: acceleration-branch noise (same stride)
    const TS* in_a;              // [n][3], or [slots][n][3] when in_ring & 1
    const TS* in_b;              // [n][3], or [slots][n][3] when in_ring & 2
    int in_ring;
    T ninv_tau_g, ninv_tau_a, earth[3];
    T mean_tol;
    int mean_max_it;
    double min_dt, max_dt;
    uint32_t* status;            // [n] or null
    int status_accumulate;       // OR into the stored word (every launch of a call but the first)
    double dt[SMOOTH_MAX_BACK];  // dt[k]: time step of the prediction redone by backward step k of this launch
};

// What a row derives from its lane index: its filter, its predicates and its LDS slice (smooth_map, ukf_host.hpp; public members
// in this order: the step loop binds them by name)
template <class T, class M, class TS> struct SmoothRow {
    static constexpr SmoothMap LY = smooth_map(M::S, M::D);
    static_assert(row_fits(M::S, M::D), "a filter fits one row");
    int l, lr, ls;          // lane of the row; clamped to a row of the matrices / an entry of the mean
    bool fvalid, live, wr;  // the row has a filter of the batch; ... that is initialised; = both: the row stores
    int64_t f;              // rows beyond the batch repeat its last filter and store nothing
    T *FAC, *RSP, *TAB, *GM, *MM, *CSM, *CSP, *MUF, *PKF, *ROT, *DUMP, *SMR, *MUP;
    const TS *Rn, *Racc;
    UKFB_DEV SmoothRow(const SmoothArgs<T, TS>& a, unsigned char* smem, int lane) {
        const RowCoords<M> rc(a.n, lane);
        l = rc.l; lr = rc.lr; ls = rc.ls; fvalid = rc.fvalid; f = rc.f;
        live = fvalid && a.initialised[f] != 0;
        wr = live;
        T* const base = row_slice<T, LY.PF>(smem, rc.g);
        FAC = base + LY.FAC; RSP = base + LY.RSP; TAB = base + LY.TAB; GM = base + LY.GM; MM = base + LY.MM;
        CSM = base + LY.CSM; CSP = base + LY.CSP; MUF = base + LY.MUF; PKF = base + LY.PKF; ROT = base + LY.ROT;
        DUMP = base + LY.DUM; SMR = base + LY.SMR; MUP = base + LY.MUP;
        Rn = a.Rn + f * a.Rn_stride;
        Racc = a.Racc + f * a.Rn_stride;
    }
};

template <class T, class M, class TS>
__global__ void __launch_bounds__(64, ROW_WAVES_PER_SIMD) ukf_smooth_kernel(const SmoothArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    constexpr SmoothMap LY = smooth_map(S, D);
    constexpr int LS = LY.LS, Q = MT<M>::Q, RT = MT<M>::RT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smooth_smem[];
    uint32_t st = ST_OK;
    int slot = a.top_slot;
    {
        // ---- the chain's start record
        const SmoothRow<T, M, TS> r(a, smooth_smem, threadIdx.x);
        st = (r.fvalid && !r.live) ? ST_UNINITIALISED : ST_OK;
        r.CSM[r.l] = T(a.start_mu[r.f * S + r.ls]);
        for (int i = r.l; i < PK; i += 16) r.CSP[i] = T(a.start_cov[r.f * PK + i]);
        wsync();
        if (r.wr) {
            if ((a.copy_top & 1) && r.l < S) a.mu_out[(int64_t(slot) * a.n + r.f) * S + r.l] = TS(r.CSM[r.l]);
            if (a.copy_top & 2)
                for (int i = r.l; i < PK; i += 16) a.cov_out[(int64_t(slot) * a.n + r.f) * PK + i] = TS(r.CSP[i]);
        }
    }
#pragma nounroll
    for (int k = 0; k < a.back; ++k) {
        // Everything derived from the lane index is invariant over the steps, and the compiler would hoist all of it out of the loop --
        // addresses, predicates, triangular indices, the noise loads: more registers than the kernel has, held across every step.  As
        // in the multi-cycle kernels the lane index passes through an opaque move in every step and its derivatives are formed again.
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        const SmoothRow<T, M, TS> row(a, smooth_smem, lane);
        const auto& [l, lr, ls, fvalid, live, wr, f, FAC, RSP, TAB, GM, MM, CSM, CSP, MUF, PKF, ROT, DUMP, SMR, MUP, Rn, Racc] = row;
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
        st |= live ? code : 0u;
        const bool dof = live && code == 0u;   // a gated step made no prediction: the chain passes through
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
            UKFB_MARK("s_predict");
            // ================================================================= 1. the prediction, redone
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
                ok1 = row_factorise<T, D, LS>(PKF, FAC, RSP, l);   // the scaled columns stay: C reads them
                T col[D];
                load_column<T, D, LS>(FAC, l, T(1), col);
                sigma_pair<T, M>(mu_r, col, xp, xm);          // lanes >= D: the centre twice (their column is zero)
            }
            sfence();
            UKFB_MARK("s_process");
            process_fast((M*)nullptr, xp, pin);
            sfence();
            process_fast((M*)nullptr, xm, pin);
            sfence();
#pragma unroll
            for (int s = 0; s < S; ++s) ref[s] = row_bcast<D>(xp[s]);   // the propagated centre starts the mean
            UKFB_MARK("s_mean");
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
            UKFB_MARK("s_deltas");
            row_publish_deltas<T, M, LS>(TAB, DUMP, l, xp, xm, ref);
            wsync();
            // Sigma^- = 1/2 sum delta delta^T + R: row lr
            T sm[D];
            row_table_row<T, D, LS>(TAB, N, lr, sm);
            sfence();
#pragma unroll
            for (int c = 0; c < D; ++c) SMR[lr * LS + c] = sm[c];   // parked in LDS until M is formed (lanes >= D: row D - 1's own bits again)
            sfence();
#pragma nounroll
            for (int c = 0; c < D; ++c) {
                const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;   // the noise's lower triangle, as the forward kernel reads it
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
            UKFB_MARK("s_cross");
            // ================================================================= 2. C = sum_j (L col j) W_j^T: row lr
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
                wsync();   // the factor of Sigma is dead
                UKFB_MARK("s_gain");
                // ============================================================= 3. G = C (Sigma^-)^-1: factor, two solves per row
                bool ok2;
                {
                    T tmp[D];
#pragma unroll
                    for (int c = 0; c < D; ++c) tmp[c] = SMR[lr * LS + c];
                    ok2 = row_factorise_row<T, D, LS>(tmp, FAC, RSP, l);
                }
                ok1 = ok1 && ok2;
                // L y = c
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    T v = cr[k];
#pragma unroll
                    for (int j = 0; j < k; ++j) v = fma(-FAC[j * LS + k], cr[j], v);
                    cr[k] = v * RSP[k];
                    sfence();
                }
                // L^T g = y
#pragma unroll
                for (int k = D - 1; k >= 0; --k) {
                    T v = cr[k];
#pragma unroll
                    for (int j = k + 1; j < D; ++j) v = fma(-FAC[k * LS + j], cr[j], v);
                    cr[k] = v * RSP[k];
                    sfence();
                }
#pragma unroll
                for (int c = 0; c < D; ++c) g_[c] = cr[c];
            }
            wsync();   // the table is dead: G and M take its place
#pragma unroll
            for (int c = 0; c < D; ++c) GM[lr * LS + c] = g_[c];   // (lanes >= D: row D - 1's own bits again)
            UKFB_MARK("s_transport");
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
            {
                const T p0 = e[RT], p1 = e[RT + 1], p2 = e[RT + 2];
                const T t = fma(p0, p0, fma(p1, p1, p2 * p2));
                const T cf = bank_jrinv_coeff(t);
                T B[9];
                B[0] = fma(cf, p0 * p0 - t, T(1)); B[1] = fma(cf, p0 * p1, T(-0.5) * p2); B[2] = fma(cf, p0 * p2, T(0.5) * p1);
                B[3] = fma(cf, p1 * p0, T(0.5) * p2); B[4] = fma(cf, p1 * p1 - t, T(1)); B[5] = fma(cf, p1 * p2, T(-0.5) * p0);
                B[6] = fma(cf, p2 * p0, T(-0.5) * p1); B[7] = fma(cf, p2 * p1, T(0.5) * p0); B[8] = fma(cf, p2 * p2 - t, T(1));
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
                const int li = lr - RT;
                const bool inrot = li >= 0 && li < 3;
                const T b0 = (li == 1) ? B[3] : ((li == 2) ? B[6] : B[0]);
                const T b1 = (li == 1) ? B[4] : ((li == 2) ? B[7] : B[1]);
                const T b2 = (li == 1) ? B[5] : ((li == 2) ? B[8] : B[2]);
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const T r0 = row_bcast<RT>(s[c]), r1 = row_bcast<RT + 1>(s[c]), r2 = row_bcast<RT + 2>(s[c]);
                    const T rot = fma(b0, r0, fma(b1, r1, b2 * r2));
                    MM[lr * LS + c] = (inrot ? rot : s[c]) - SMR[lr * LS + c];   // M = Sigma^t - Sigma^-
                }
            }
            wsync();
            UKFB_MARK("s_cov");
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
                // (G M) row lr through LDS (the factor of Sigma^- is dead): the second product indexes it by a loop variable
#pragma unroll
                for (int c = 0; c < D; ++c) FAC[lr * LS + c] = tr[c];
                sfence();
#pragma nounroll
                for (int j = 0; j < D; ++j) {
                    const T tj = FAC[lr * LS + j];
                    const T* gc = GM + j;
#pragma unroll
                    for (int c = 0; c < D; ++c) sg[c] = fma(tj, gc[c * LS], sg[c]);   // the rows other lanes wrote
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
            wsync();   // G and M are dead
            UKFB_MARK("s_commit");
            // ================================================================= 6. commit: applyDelta(mu, Sigma~, delta)
            T mnew[S];
            const bool ok3 = row_apply_delta<T, M, LS>(FAC, TAB, MUF, DUMP, l, lr, del, sg, mu_r, mnew);   // (mu_r: reloaded, not kept live across the step)
            const bool good = dof && ok1 && ok3;
            st |= (dof && !good) ? ST_ERR_CHOLESKY : 0u;
            st |= (dof && good && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
            // the chain moves on: the smoothed record, or (a failure) the filtered one bit for bit; a gated row keeps it
            // (the store block of the updates, but a failure's values come from LDS entry by entry)
            {
                T v = good ? mnew[0] : mu_r[0];
#pragma unroll
                for (int s = 1; s < S; ++s) v = (ls == s) ? (good ? mnew[s] : mu_r[s]) : v;
                T* dst = (dof && l < S) ? (CSM + l) : DUMP;
                *dst = v;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const int idx = lr * (lr + 1) / 2 + c;
                    const bool own = dof && l < D && c <= l;
                    const T fv = PKF[own ? idx : 0];
                    T* dc = own ? (CSP + idx) : DUMP;
                    *dc = good ? sg[c] : fv;
                }
            }
            wsync();
        }
        UKFB_MARK("s_store");
        // ---- the smoothed record of this step leaves
        if (wr) {
            if (l < S) a.mu_out[rec * S + l] = TS(CSM[l]);
            if (a.cov_out)
                for (int i = l; i < PK; i += 16) a.cov_out[rec * PK + i] = TS(CSP[i]);
        }
        wsync();
    }
    {
        const SmoothRow<T, M, TS> r(a, smooth_smem, threadIdx.x);
        if (r.wr) {
            if (a.end_cov)
                for (int i = r.l; i < PK; i += 16) a.end_cov[r.f * PK + i] = TS(r.CSP[i]);
            if (a.status && r.l == 0) a.status[r.f] = a.status_accumulate ? (a.status[r.f] | st) : st;
        } else if (r.fvalid && a.status && r.l == 0) {
            a.status[r.f] = st;   // UNINITIALISED
        }
    }
}

}  // namespace ukfb
