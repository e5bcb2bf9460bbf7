// ukf_innovation.hpp -- innovation statistics without an update: the first half of ukfom's update (predicted measurement
// z-bar, innovation covariance S, innovation nu = z (-) z-bar, squared Mahalanobis distance, measurement log-likelihood)
// for up to 32 candidate samples per filter, and the nearest candidate inside the chi-square gate.  READ-ONLY: the kernel
// has no pointer to the engine's state through which it could store.
//
// Layout: the tuned one (ukf_kernel16.hpp) -- one filter per 16-lane DPP row, four per wavefront, one wavefront per
// workgroup -- and the same device functions, so that a candidate's d^2 is the number the update's own gate compares:
//  * per filter, once: mean and the covariance entries the model reads, straight from HBM (no packed-covariance staging).
//    The eight sub-state selections of PoseWithVelocity use the closed form of the unscented transform of a linear map,
//    as the update kernels do (z-bar = mu[sel], S = Sigma[sel][sel] + Q: six covariance entries, no factorisation).  The
//    orientation-dependent models (PoseUKF OrientationMeasurement, OrientationUKF body velocity) factorise the
//    MT<M>::ZCOLS = 6 leading columns (chol16), spread the sigma pairs over the lanes, take the mean (SO(3): ukfom's
//    iteration with mean_tol / mean_max_iter) and sum S over the row.
//  * S^-1 (inverse3) and det S once per filter; ln det S by the compiler's log.
//  * candidates: LANE k scores candidate k (k + 16 in a second pass), so that up to sixteen candidates cost one (-), one
//    quadratic form and up to five stores of a single lane each; the nearest gated candidate is a 16-step row scan
//    (strictly-less: ties go to the lower index, NaN never wins).
//  * LDS: the six factor columns (stride 14) and the mean, 100 scalars per filter: 1 600 B (fp32) / 3 200 B (fp64) per
//    workgroup = 2 / 3 allocation granules of 1 280 B, far from limiting occupancy.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
// Per-filter model ids take the same kernel: both paths are wave-uniform branches.
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

template <class TS> struct InnovArgs {
    int64_t n;                   // filters
    const TS* mu;                // [n][S]
    const TS* cov;               // [n][PK]
    const uint8_t* initialised;  // [n]
    int meas_uniform;
    const int32_t* meas;         // [n] or null
    int candidates;              // 1 .. 32
    const TS* z;                 // [candidates][n][3]
    const TS* Q;                 // [n][9], or [9] when q_uniform
    int q_uniform;
    TS mean_tol;
    int mean_max_it;
    TS gate_chi2;                // < 0: every finite candidate is eligible
    // outputs, any may be null
    TS* z_pred;                  // [n][4]
    TS* S;                       // [n][9]
    TS* innov;                   // [candidates][n][3]
    TS* maha;                    // [candidates][n]
    TS* loglik;                  // [candidates][n]
    int32_t* best;               // [n]
    uint32_t* status;            // [n]
};

constexpr int UKFB_MAX_CANDIDATES = 32;

template <class M> struct InnovLayout {
    static constexpr int LS = 14;                       // column stride of the factor, as Layout16
    static constexpr int MUS = MT<M>::ZCOLS * LS;       // mean staging behind the ZCOLS factor columns
    static constexpr int PF = MUS + 16;                 // 100 scalars: the four slices start on different banks
    static_assert(M::S <= 16 && M::D <= LS, "a filter fits one row");
};

template <class T, class M, class TS>
__global__ void __launch_bounds__(64) ukf_innovation_kernel(const InnovArgs<TS> a) {
    constexpr int S = M::S, D = M::D, N = 2 * D + 1, PK = D * (D + 1) / 2;
    using LY = InnovLayout<M>;
    constexpr int LS = LY::LS, Q = MT<M>::Q, RT = MT<M>::RT, ZC = MT<M>::ZCOLS;
    constexpr int FPW = 4;
    __shared__ __attribute__((aligned(16))) T smem[FPW * LY::PF];

    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int64_t wg0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * FPW;
    const int64_t n_here = a.n - wg0;
    const int n_wg = int(n_here < FPW ? n_here : int64_t(FPW));
    const bool fvalid = g < n_wg;
    const int64_t f = wg0 + (fvalid ? g : (n_wg - 1));   // rows beyond the batch repeat its last filter and store nothing
    T* Lc = smem + g * LY::PF;
    T* MUS = Lc + LY::MUS;
    const int K = a.candidates;

    // ---- per-filter loads
    const uint8_t init_b = a.initialised[f];
    const int mid = a.meas ? a.meas[f] : a.meas_uniform;
    const TS* covf = a.cov + f * PK;
    MUS[l] = T(a.mu[f * S + ((l < S) ? l : (S - 1))]);
    T Qm[9];
    {
        const TS* qp = a.Q + (a.q_uniform ? int64_t(0) : f * 9);
#pragma unroll
        for (int k = 0; k < 9; ++k) Qm[k] = T(qp[k]);
    }
    const bool live = init_b != 0;
    const bool act = M::meas_valid(mid);
    const bool do_u = live && act;
    uint32_t st = ST_OK;
    st |= live ? 0u : ST_UNINITIALISED;
    st |= (live && !act) ? ST_INACTIVE : 0u;
    const int midc = act ? mid : (M::MODEL == 0 ? 0 : 9);
    const int m = M::meas_dim(midc);
    const bool so3 = M::meas_is_so3(midc);
    const bool need_q = so3 || (M::MODEL == 1);
    wsync();

    // ---- measurement statistics of the filter: z-bar (zref; a quaternion for SO(3)), S (Sm, identity on the unused dimensions)
    bool ok1 = true, zconv = true;
    T Sm[9], zref[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int k = 0; k < 9; ++k) Sm[k] = (k % 4 == 0) ? T(1) : T(0);
    if constexpr (MT<M>::HAS_EUCLID_MEAS) {
        // sub-state selections: the unscented transform of a linear map is exact (ukf_kernel16.hpp, "u_stats")
        const unsigned long long sel[3] = {MT<M>::SEL0, MT<M>::SEL1, MT<M>::SEL2};
        int ti[3];
        bool used[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int sk = int((sel[k] >> (4 * midc)) & 15ull);
            used[k] = sk != 15;
            const int si = used[k] ? sk : 0;
            ti[k] = (si < Q) ? si : (si - 1);
            const T m0 = MUS[si];
            zref[k] = used[k] ? m0 : T(0);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const int hi = ti[r] > ti[c] ? ti[r] : ti[c], lo = ti[r] > ti[c] ? ti[c] : ti[r];
                const T sp = T(covf[hi * (hi + 1) / 2 + lo]);
                const T pad = (r == c) ? T(1) : T(0);
                const bool u = used[r] && used[c];
                Sm[r * 3 + c] = u ? (sp + Qm[r * 3 + c]) : pad;
                if (c < r) Sm[c * 3 + r] = u ? (sp + Qm[c * 3 + r]) : pad;
            }
    }
    if (wave_any(need_q)) {
        // orientation-dependent models: the sigma-point path of ukfom::update up to S (ukf_kernel16.hpp, "u_stats")
        bool okg;
        T rs;
        {
            T arow[D];
            const int lr = (l < D) ? l : (D - 1);
            const TS* p = covf + lr * (lr + 1) / 2;   // row lr, entries 0 .. ZC-1 (beyond the diagonal: the next row's, finite, masked by chol16)
#pragma unroll
            for (int j = 0; j < D; ++j) arow[j] = (j < ZC) ? T(p[j]) : T(0);
            rs = chol16<T, D, LS, ZC>(arow, Lc, l, okg);
            wsync();
        }
        const bool has_pair = l < D;
        T zp[4], zm[4], z0[4];
        {
            const bool zcol = l < ZC;
            const T w = zcol ? rs : T(0);
            const T* colp = Lc + (zcol ? l : (ZC - 1)) * LS;
            const T q0[4] = {MUS[Q], MUS[Q + 1], MUS[Q + 2], MUS[Q + 3]};
            const T cr[3] = {colp[RT] * w, colp[RT + 1] * w, colp[RT + 2] * w};
            T e[4], qp[4], qm[4];
            so3_exp_fast(cr, T(1), e);
            quat_mul_pm(q0, e, qp, qm);
            MT<M>::gen_measure(qp, qm, q0, MUS, colp, w, zp, zm, z0);
        }
        T zr4[4] = {z0[0], z0[1], z0[2], z0[3]};
        bool zc = true;
        if (wave_any(so3 && do_u && okg)) {
            bool active = so3 && do_u && okg;
            int it = 0;
            while (wave_any(active)) {
                T rp[3], rm[3], r0v[3], mr[3];
                rot_minus(zp, zr4, rp);
                rot_minus(zm, zr4, rm);
                rot_minus(z0, zr4, r0v);
                T m2 = T(0);
#pragma unroll
                for (int k = 0; k < 3; ++k) mr[k] = has_pair ? (rp[k] + rm[k]) : T(0);
                row_allreduce_n<T, 3>(mr);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    mr[k] = (mr[k] + r0v[k]) * (T(1) / T(N));
                    m2 += mr[k] * mr[k];
                }
                T e[4], nq[4];
                so3_exp_fast(mr, T(1), e);
                quat_mul(zr4, e, nq);
#pragma unroll
                for (int k = 0; k < 4; ++k) zr4[k] = active ? nq[k] : zr4[k];
                const bool more = m2 > T(a.mean_tol) * T(a.mean_tol);
                const bool capped = more && (it + 1 >= a.mean_max_it);
                it += (active && more) ? 1 : 0;
                zc = zc && !(active && capped);
                active = active && more && !capped;
            }
        }
        {
            T zr[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) zr[k] = has_pair ? ((zp[k] - z0[k]) + (zm[k] - z0[k])) : T(0);
            row_allreduce_n<T, 3>(zr);
#pragma unroll
            for (int k = 0; k < 3; ++k) zr[k] = z0[k] + zr[k] * (T(1) / T(N));
#pragma unroll
            for (int k = 0; k < 3; ++k) zr4[k] = so3 ? zr4[k] : zr[k];
            zr4[3] = so3 ? zr4[3] : T(0);
        }
        T dzp[3], dzm[3], dz0[3];
        {
            T a3[3] = {T(0), T(0), T(0)}, b3[3] = {T(0), T(0), T(0)}, c3[3] = {T(0), T(0), T(0)};
            if (wave_any(so3)) {
                rot_minus(zp, zr4, a3);
                rot_minus(zm, zr4, b3);
                rot_minus(z0, zr4, c3);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dzp[k] = so3 ? a3[k] : (zp[k] - zr4[k]);
                dzm[k] = so3 ? b3[k] : (zm[k] - zr4[k]);
                dz0[k] = so3 ? c3[k] : (z0[k] - zr4[k]);
            }
        }
        T Sg[9];
        {
            T u6[6];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) u6[r * (r + 1) / 2 + c] = has_pair ? fma(dzp[r], dzp[c], dzm[r] * dzm[c]) : T(0);
            row_allreduce_n<T, 6>(u6);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c)
                    u6[r * (r + 1) / 2 + c] = T(0.5) * (u6[r * (r + 1) / 2 + c] + dz0[r] * dz0[c]);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int hi = r > c ? r : c, lo = r > c ? c : r;
                    const T pad = (r == c) ? T(1) : T(0);
                    Sg[r * 3 + c] = (r >= m || c >= m) ? pad : (u6[hi * (hi + 1) / 2 + lo] + Qm[r * 3 + c]);
                }
        }
        ok1 = need_q ? okg : ok1;
        zconv = need_q ? zc : zconv;
#pragma unroll
        for (int k = 0; k < 9; ++k) Sm[k] = need_q ? Sg[k] : Sm[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) zref[k] = need_q ? zr4[k] : zref[k];
    }

    // ---- S^-1, det S; S must be positive definite (leading minors; NaN fails every comparison)
    T Si[9];
    inverse3(Sm, Si);
    const T c00 = Sm[4] * Sm[8] - Sm[5] * Sm[7], c10 = Sm[7] * Sm[2] - Sm[8] * Sm[1], c20 = Sm[1] * Sm[5] - Sm[2] * Sm[4];
    const T det = c00 * Sm[0] + c10 * Sm[3] + c20 * Sm[6];
    const bool s_pd = (Sm[0] > T(0)) && (Sm[0] * Sm[4] - Sm[1] * Sm[3] > T(0)) && (det > T(0)) && m_finite(det);
    st |= (do_u && !(ok1 && s_pd)) ? ST_ERR_CHOLESKY : 0u;
    st |= (do_u && ok1 && s_pd && !zconv) ? ST_WARN_MEAN_NOCONV : 0u;
    const bool good = do_u && ok1 && s_pd;
    const T lognorm = m_log(det) + T(m) * T(1.8378770664093454835606594728112);   // ln det S + m ln 2 pi

    // ---- candidates: lane k scores candidate k
    const T gate = T(a.gate_chi2);
    T bestv = T(__builtin_inff());
    int besti = -1;
    float nfin = 0.0f;
    const int passes = (K + 15) >> 4;
    for (int p = 0; p < passes; ++p) {
        const int k = l + 16 * p;
        const bool kv = k < K;
        const TS* zk = a.z + (int64_t(kv ? k : 0) * a.n + f) * 3;
        const T zin[3] = {T(zk[0]), T(zk[1]), T(zk[2])};
        const bool fin = m_finite(zin[0]) && (m < 2 || m_finite(zin[1])) && (m < 3 || m_finite(zin[2]));
        T inn[3];
        {
            T d3[3] = {T(0), T(0), T(0)};
            if (wave_any(so3)) {
                T qe[4];
                so3_exp_fast(zin, T(1), qe);   // RotationType(SO3::exp(mu)), PoseUKF.cpp:135
                rot_minus(qe, zref, d3);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) inn[c] = so3 ? d3[c] : ((c < m) ? (zin[c] - zref[c]) : T(0));
        }
        T d2 = T(0);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) d2 += inn[r] * Si[r * 3 + c] * inn[c];
        const bool valid = good && fin;
        d2 = valid ? d2 : m_nan<T>();
        const T ll = T(-0.5) * (d2 + lognorm);
        nfin += (kv && fin) ? 1.0f : 0.0f;
        if (kv && fvalid) {
            const int64_t o = int64_t(k) * a.n + f;
            if (a.innov) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.innov[o * 3 + c] = TS((valid && c < m) ? inn[c] : ((c < m) ? m_nan<T>() : T(0)));
            }
            if (a.maha) a.maha[o] = TS(d2);
            if (a.loglik) a.loglik[o] = TS(ll);
        }
        // nearest eligible candidate of the row: strictly less, so equal distances keep the lower index
        const bool elig = kv && valid && m_finite(d2) && ((gate < T(0)) || (d2 <= gate));
        const T key = elig ? d2 : T(__builtin_inff());
        static_for<0, 16>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            const T v = row_bcast<c>(key);
            const bool lt = v < bestv;
            bestv = lt ? v : bestv;
            besti = lt ? (c + 16 * p) : besti;
        });
    }
    nfin = row_allreduce(nfin);
    st |= (good && nfin == 0.0f) ? ST_ERR_NONFINITE_MEAS : 0u;

    // ---- per-filter outputs
    if (fvalid) {
        const T nanv = m_nan<T>();
        if (a.z_pred && l < 4) {
            T v = zref[0];
#pragma unroll
            for (int k = 1; k < 4; ++k) v = (l == k) ? zref[k] : v;
            a.z_pred[f * 4 + l] = TS(good ? v : nanv);
        }
        if (a.S && l < 9) {
            T v = T(0);
#pragma unroll
            for (int k = 0; k < 9; ++k) v = (l == k) ? ((k / 3 < m && k % 3 < m) ? Sm[k] : T(0)) : v;
            a.S[f * 9 + l] = TS(good ? v : nanv);
        }
        if (l == 0) {
            if (a.best) a.best[f] = good ? besti : -1;
            if (a.status) a.status[f] = st;
        }
    }
}

// z_sel[i] = z[best[i]][i], meas_sel[i] = best[i] < 0 ? -1 : model(i): what ukfb_update_dev needs to finish nearest-neighbour
// association on the device
template <class TS>
__global__ void select_candidates_kernel(int64_t n, int candidates, const int32_t* best, int meas_uniform, const int32_t* meas,
                                         const TS* z, TS* z_sel, int32_t* meas_sel) {
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int b = best[i];
    const bool have = b >= 0 && b < candidates;
    const TS* zk = z + (int64_t(have ? b : 0) * n + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) z_sel[i * 3 + c] = have ? zk[c] : TS(0);
    if (meas_sel) meas_sel[i] = have ? (meas ? meas[i] : meas_uniform) : -1;
}

}  // namespace ukfb
