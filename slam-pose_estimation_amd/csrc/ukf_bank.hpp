// ukf_bank.hpp -- filter banks on the device: an engine of `capacity` filters read as capacity / M TRACKS of M HYPOTHESES
// (track-major: hypothesis j of track t is filter t * M + j, so a track's records are contiguous in HBM).
//   bank_combine  mixture moments of every track (one estimate per track); READ-ONLY on the engine
//   bank_mix      the IMM interaction step: every hypothesis replaced by the mixture of all M under the mixing weights
//   bank_weights  log-likelihoods -> normalised log-weights and weights (an M-wide log-sum-exp)
// Definitions: include/ukf_batch.h ("filter banks"), DESIGN.md 4.14.
//
// Layout: the tuned one (ukf_kernel16.hpp) -- one track per 16-lane DPP row, four per wavefront, one wavefront per workgroup.
//  * the M records of a track (mean, packed covariance) cross HBM once, into LDS (bank_track_scalars of ukf_host.hpp); mix
//    computes its M outputs from that copy and stores each as soon as it is complete.
//  * mean: LANE j < M holds hypothesis j and takes ITS logarithm against the reference, one per trip; the weighted deltas are
//    summed over the row (ukfom's stopping rule with mean_tol / mean_max_iter, as the sigma-point means).
//  * covariance: lane l < D owns row l of J Sigma_j J^T and of the accumulator, the hypotheses are looped.  J is the identity
//    but for the 3x3 block Jr^-1(phi) on the rotation, so the congruence is a 3-column product inside the lane and a 3-row
//    product across the rotation's three lanes (row broadcasts).
//  * a hypothesis of weight exactly 0 is skipped by selects: its state never reaches a result.
//  * a converged track rides along unchanged while a wave-mate iterates: no track's bits depend on its neighbours.
//  * TS (storage) / T (compute) as in ukf_kernel16: TS = float with T = double is the wide-arithmetic mode.
#pragma once

#include "ukf_row.hpp"

namespace ukfb {

constexpr uint32_t ST_ERR_WEIGHTS = 1u << 10;

template <class T, class TS> struct BankArgs {
    int64_t tracks;
    int hyp;                     // M, 2 ... 8
    const TS* mu_in;             // [tracks * M][S]
    const TS* cov_in;            // [tracks * M][PK]
    const uint8_t* initialised;  // [tracks * M]
    const TS* w;                 // [tracks * M]
    T mean_tol;
    int mean_max_it;
    T sum_tol;                   // 16 M eps of the storage precision
    // combine: one record per track (cov_out may be null); mix: the engine's own arrays, one record per hypothesis
    TS* mu_out;
    TS* cov_out;
    TS* w_pred;                  // mix: [tracks * M]
    uint32_t* status;            // [tracks], may be null
    T Pi[BANK_GROUP_SCALARS];    // mix: transition [M][M], row-major
};

// c(theta) of Jr^-1(phi) = I + [phi]x / 2 + c [phi]x^2, as a function of t = theta^2:
// c = (1 - (theta/2) cot(theta/2)) / t = (sinc(theta/2) - cos(theta/2)) / (t sinc(theta/2)) above t = 0.25: the half-angle form
// has no cancellation towards theta = pi (the edge of so3_log's range, c = 1/pi^2) and no zero denominator below 2 pi, where
// Jr^-1 has its pole; the full-angle form (2 sinc - 1 - cos) / (2 t sinc) is 0/0 at pi.  At and below t = 0.25 the series: its
// remainder there is 3e-15 absolute, 4e-14 = 180 eps(fp64) of c, and falls like t^6; its effect on Jr^-1 is c t.
// tests/test_gpu_jacobian_primitives.py holds c and Jr^-1 to 40-digit references from t = 0 to fl(pi)^2 and lists the errors.
template <class T> UKFB_DEV T bank_jrinv_coeff(T t) {
    T c = T(691. / 1307674368000.);
    c = fma(c, t, T(1. / 47900160.));
    c = fma(c, t, T(1. / 1209600.));
    c = fma(c, t, T(1. / 30240.));
    c = fma(c, t, T(1. / 720.));
    c = fma(c, t, T(1. / 12.));
    const bool big = !(t <= T(0.25));
    if (wave_any(big)) {
        T ch, sh;
        cos_sinc_fast(big ? T(0.25) * t : T(0.25), ch, sh);   // cos(theta / 2), sinc(theta / 2)
        const T closed = (sh - ch) * fast_rcp(t * sh);
        c = big ? closed : c;
    }
    return c;
}

// x (-) y of the engine's manifold; a rotation with the reference's own bits gives exactly zero (x (-) x = 0: with fused
// multiply-adds conj(q) q has a vector part of rounding size, which would move a one-hot mixture off its hypothesis)
template <class T, class M> UKFB_DEV void bank_boxminus(const T (&x)[M::S], const T (&y)[M::S], T (&d)[M::D]) {
    constexpr int Q = MT<M>::Q, RT = MT<M>::RT;
    M::boxminus(x, y, d);
    const bool same = x[Q] == y[Q] && x[Q + 1] == y[Q + 1] && x[Q + 2] == y[Q + 2] && x[Q + 3] == y[Q + 3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[RT + k] = same ? T(0) : d[RT + k];
}

// Mixture moments of one track (one 16-lane row).  MUL [Mh][S], CVL [Mh][PK]: the track's records in LDS; DEL [Mh][D]: scratch
// of the row.  wl: the weight of hypothesis l on lane l (anything beyond Mh).  On return every lane holds the mean in ref and
// lane l < D row l of the covariance in acc (entries 0 .. l are the ones stored).
template <class T, class M>
UKFB_DEV void bank_mixture(const T* MUL, const T* CVL, T* DEL, int Mh, int l, T wl, T tol, int max_it, T (&ref)[M::S],
                           T (&acc)[M::D], bool& conv) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2, RT = MT<M>::RT;
    const bool used = (l < Mh) && (wl != T(0));
    const int jl = (l < Mh) ? l : (Mh - 1);
    T x[S];
#pragma unroll
    for (int k = 0; k < S; ++k) x[k] = MUL[jl * S + k];
    // the reference starts at the hypothesis of the largest weight (strictly greater: ties keep the lower index)
    int js = 0;
    {
        const T key = used ? wl : T(-1);
        T best = T(-1);
        static_for<0, BANK_MAX_HYPOTHESES>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            const T v = row_bcast<c>(key);
            const bool gt = v > best;
            best = gt ? v : best;
            js = gt ? c : js;
        });
    }
#pragma unroll
    for (int k = 0; k < S; ++k) ref[k] = MUL[js * S + k];
    // mean: d = sum_j w_j (mu_j (-) ref), ref <- ref (+) d; do ... while (|d| > tol && ++it < max_it)
    conv = true;
    {
        bool active = true;
        int it = 0;
        while (wave_any(active)) {
            T d[D];
            bank_boxminus<T, M>(x, ref, d);
#pragma unroll
            for (int k = 0; k < D; ++k) d[k] = used ? wl * d[k] : T(0);
            row_allreduce_n<T, D, 3>(d);   // lanes 8 .. 15 hold no hypothesis
            T m2 = T(0);
#pragma unroll
            for (int k = 0; k < D; ++k) m2 = fma(d[k], d[k], m2);
            T nr[S];
#pragma unroll
            for (int k = 0; k < S; ++k) nr[k] = ref[k];
            M::boxplus(nr, d);
            const bool move = active && (m2 != T(0));
#pragma unroll
            for (int k = 0; k < S; ++k) ref[k] = move ? nr[k] : ref[k];
            const bool more = m2 > tol * tol;
            const bool capped = more && (it + 1 >= max_it);
            it += (active && more) ? 1 : 0;
            conv = conv && !(active && capped);
            active = active && more && !capped;
        }
    }
    // deltas of the hypotheses to the mean and their weights, lane j's into DEL[j]
    constexpr int DS = D + 1;
    {
        T d[D];
        bank_boxminus<T, M>(x, ref, d);
        if (l < Mh) {
#pragma unroll
            for (int k = 0; k < D; ++k) DEL[l * DS + k] = d[k];
            DEL[l * DS + D] = wl;
        }
    }
    wsync();
    // covariance: sum_j w_j (J_j Sigma_j J_j^T + delta_j delta_j^T), lane l owns row l
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = T(0);
    const int lr = (l < D) ? l : (D - 1);
    const int li = lr - RT;
    const bool inrot = li >= 0 && li < 3;
    for (int j = 0; j < Mh; ++j) {
        const T wj = DEL[j * DS + D];
        T dj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) dj[k] = DEL[j * DS + k];
        // B = Jr^-1(phi) = I + [phi]x / 2 + c ([phi phi^T] - |phi|^2 I), row-major
        const T p0 = dj[RT], p1 = dj[RT + 1], p2 = dj[RT + 2];
        const T t = fma(p0, p0, fma(p1, p1, p2 * p2));
        const T cf = bank_jrinv_coeff(t);
        T B[9];
        B[0] = fma(cf, p0 * p0 - t, T(1)); B[1] = fma(cf, p0 * p1, T(-0.5) * p2); B[2] = fma(cf, p0 * p2, T(0.5) * p1);
        B[3] = fma(cf, p1 * p0, T(0.5) * p2); B[4] = fma(cf, p1 * p1 - t, T(1)); B[5] = fma(cf, p1 * p2, T(-0.5) * p0);
        B[6] = fma(cf, p2 * p0, T(-0.5) * p1); B[7] = fma(cf, p2 * p1, T(0.5) * p0); B[8] = fma(cf, p2 * p2 - t, T(1));
        // row lr of Sigma_j (symmetric, packed lower triangle)
        T s[D];
        const T* Cj = CVL + j * PK;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int hi = lr > c ? lr : c, lo = lr > c ? c : lr;
            s[c] = Cj[hi * (hi + 1) / 2 + lo];
        }
        // (Sigma J^T): the three rotation columns of the lane's row
        {
            const T s0 = s[RT], s1 = s[RT + 1], s2 = s[RT + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i) s[RT + i] = fma(s0, B[3 * i], fma(s1, B[3 * i + 1], s2 * B[3 * i + 2]));
        }
        // J (Sigma J^T): the three rotation rows are combinations of the rows of lanes RT .. RT + 2
        const T b0 = (li == 1) ? B[3] : ((li == 2) ? B[6] : B[0]);
        const T b1 = (li == 1) ? B[4] : ((li == 2) ? B[7] : B[1]);
        const T b2 = (li == 1) ? B[5] : ((li == 2) ? B[8] : B[2]);
        const T dl = DEL[j * DS + lr];   // the lane's own component of delta_j
        const bool usej = wj != T(0);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const T r0 = row_bcast<RT>(s[c]), r1 = row_bcast<RT + 1>(s[c]), r2 = row_bcast<RT + 2>(s[c]);
            const T rot = fma(b0, r0, fma(b1, r1, b2 * r2));
            const T a = inrot ? rot : s[c];
            acc[c] = usej ? fma(wj, fma(dl, dj[c], a), acc[c]) : acc[c];
        }
    }
}

// Loads the records of the row's track into LDS, validates it (status bits) and returns the weight of hypothesis l on lane l
template <class T, class M, class TS>
UKFB_DEV T bank_stage(const BankArgs<T, TS>& a, int64_t trk, int l, T* MUL, T* CVL, uint32_t& st) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2;
    const int Mh = a.hyp;
    const int64_t f0 = trk * Mh;
    for (int i = l; i < Mh * S; i += 16) MUL[i] = T(a.mu_in[f0 * S + i]);
    for (int i = l; i < Mh * PK; i += 16) CVL[i] = T(a.cov_in[f0 * PK + i]);
    const int jl = (l < Mh) ? l : (Mh - 1);
    const T wl = T(a.w[f0 + jl]);
    const bool uninit = a.initialised[f0 + jl] == 0;
    const bool wbad = !(wl >= T(0)) || !m_finite(wl);
    T sum = (l < Mh) ? wl : T(0);
    if constexpr (sizeof(T) == 8) sum = row_allreduce<3>(sum);
    else sum = row_allreduce(sum);
    st = ST_OK;
    st |= row_any(uninit) ? ST_UNINITIALISED : 0u;
    st |= (row_any(wbad) || !(m_abs(sum - T(1)) <= a.sum_tol)) ? ST_ERR_WEIGHTS : 0u;
    return wl;
}

template <class T, class M> struct BankSlices {
    static constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2;
    T *MUL, *CVL, *DEL, *OUT;
    UKFB_DEV BankSlices(T* smem, int g, int Mh) {
        T* base = smem + BANK_GROUP_SCALARS + g * bank_track_scalars(S, D, Mh);
        MUL = base;
        CVL = MUL + Mh * S;
        DEL = CVL + Mh * PK;
        OUT = DEL + Mh * (D + 1);
    }
};

// mean (every lane) and covariance rows (lane l < D) into the row's output record in LDS
template <class T, class M> UKFB_DEV void bank_publish(T* OUT, int l, const T (&ref)[M::S], const T (&acc)[M::D]) {
    constexpr int S = M::S, D = M::D;
#pragma unroll
    for (int k = 0; k < S; ++k) OUT[k] = ref[k];   // the same bits from every lane of the row
#pragma unroll
    for (int c = 0; c < D; ++c)
        if (l < D && c <= l) OUT[S + l * (l + 1) / 2 + c] = acc[c];
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64) ukf_bank_combine_kernel(const BankArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2, TPG = BANK_TRACKS_PER_GROUP;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_smem[];
    T* smem = reinterpret_cast<T*>(bank_smem);
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int Mh = a.hyp;
    const int64_t t0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * TPG;
    const int64_t n_here = a.tracks - t0;
    const int n_wg = int(n_here < TPG ? n_here : int64_t(TPG));
    const bool tvalid = g < n_wg;
    const int64_t trk = t0 + (tvalid ? g : (n_wg - 1));   // rows beyond the batch repeat its last track and store nothing
    const BankSlices<T, M> ls(smem, g, Mh);
    uint32_t st;
    const T wl = bank_stage<T, M, TS>(a, trk, l, ls.MUL, ls.CVL, st);
    wsync();
    T ref[S], acc[D];
    bool conv;
    const bool bad = st != ST_OK;
    // a failing track is mixed under the one-hot on its hypothesis 0 (one trip; nothing of it is stored): it must not keep
    // its wave-mates iterating on weights that are no distribution
    const T wm = bad ? ((l == 0) ? T(1) : T(0)) : wl;
    bank_mixture<T, M>(ls.MUL, ls.CVL, ls.DEL, Mh, l, wm, a.mean_tol, a.mean_max_it, ref, acc, conv);
    st |= (!bad && !conv) ? ST_WARN_MEAN_NOCONV : 0u;
    bank_publish<T, M>(ls.OUT, l, ref, acc);
    wsync();
    if (tvalid) {
        const T nanv = m_nan<T>();
        if (l < S) a.mu_out[trk * S + l] = TS(bad ? nanv : ls.OUT[l]);
        if (a.cov_out)
            for (int i = l; i < PK; i += 16) a.cov_out[trk * PK + i] = TS(bad ? nanv : ls.OUT[S + i]);
        if (a.status && l == 0) a.status[trk] = st;
    }
}

template <class T, class M, class TS>
__global__ void __launch_bounds__(64) ukf_bank_mix_kernel(const BankArgs<T, TS> a) {
    constexpr int S = M::S, D = M::D, PK = D * (D + 1) / 2, TPG = BANK_TRACKS_PER_GROUP;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_smem[];
    T* smem = reinterpret_cast<T*>(bank_smem);
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int Mh = a.hyp;
    const int64_t t0 = int64_t(group_of_block(blockIdx.x, gridDim.x)) * TPG;
    const int64_t n_here = a.tracks - t0;
    const int n_wg = int(n_here < TPG ? n_here : int64_t(TPG));
    const bool tvalid = g < n_wg;
    const int64_t trk = t0 + (tvalid ? g : (n_wg - 1));
    const BankSlices<T, M> ls(smem, g, Mh);
    smem[lane] = a.Pi[lane];
    uint32_t st;
    const T wl = bank_stage<T, M, TS>(a, trk, l, ls.MUL, ls.CVL, st);
    wsync();
    const bool bad = st != ST_OK;
    const bool usedw = (l < Mh) && (wl != T(0));
    const int jl = (l < Mh) ? l : (Mh - 1);
    T wpred = wl;
    bool conv_all = true;
    for (int i = 0; i < Mh; ++i) {
        // c_i = sum_j Pi[j][i] w_j, w_{j|i} = Pi[j][i] w_j / c_i; c_i = 0: hypothesis i keeps its state
        const T u = usedw ? smem[jl * Mh + i] * wl : T(0);
        T ci;
        if constexpr (sizeof(T) == 8) ci = row_allreduce<3>(u);
        else ci = row_allreduce(u);
        const bool go = ci > T(0);
        const T wji = (go && !bad) ? (u / ci) : ((l == i) ? T(1) : T(0));   // nothing to mix: the one-hot on i, one trip
        wpred = (l == i) ? ci : wpred;
        T ref[S], acc[D];
        bool conv;
        bank_mixture<T, M>(ls.MUL, ls.CVL, ls.DEL, Mh, l, wji, a.mean_tol, a.mean_max_it, ref, acc, conv);
        bank_publish<T, M>(ls.OUT, l, ref, acc);
        wsync();
        const bool store = tvalid && !bad && go;
        conv_all = conv_all && (conv || !go);
        if (store) {
            const int64_t f = trk * Mh + i;
            if (l < S) a.mu_out[f * S + l] = TS(ls.OUT[l]);
            for (int k = l; k < PK; k += 16) a.cov_out[f * PK + k] = TS(ls.OUT[S + k]);
        }
        wsync();
    }
    st |= (!bad && !conv_all) ? ST_WARN_MEAN_NOCONV : 0u;
    if (tvalid) {
        if (l < Mh) a.w_pred[trk * Mh + l] = TS(bad ? wl : wpred);
        if (a.status && l == 0) a.status[trk] = st;
    }
}

// logw_out = logw_in + loglik - logsumexp_j(logw_in + loglik), w_out = exp(logw_out); one thread per track
template <class T, class TS> struct BankWeightArgs {
    int64_t tracks;
    int hyp;
    const TS* logw_in;   // [tracks * M] or null (uniform)
    const TS* loglik;    // [tracks * M] or null (normalise only); NaN = the hypothesis is dead
    TS* logw_out;        // [tracks * M]
    TS* w_out;           // [tracks * M] or null
    uint32_t* status;    // [tracks] or null
};

template <class T, class TS> __global__ void __launch_bounds__(256) ukf_bank_weights_kernel(const BankWeightArgs<T, TS> a) {
    const int64_t trk = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (trk >= a.tracks) return;
    const int Mh = a.hyp;
    const int64_t f0 = trk * Mh;
    const T ninf = -T(__builtin_inff());
    // pass 0: logw_in + loglik; pass 1 (every hypothesis dead): logw_in on its own; pass 2 (still nothing): uniform
    uint32_t st = ST_OK;
    T mx = ninf;
    int pass = 0;
    for (; pass < 3; ++pass) {
        mx = ninf;
        for (int j = 0; j < Mh; ++j) {
            T v = (a.logw_in && pass < 2) ? T(a.logw_in[f0 + j]) : T(0);
            if (a.loglik && pass == 0) v += T(a.loglik[f0 + j]);
            v = (v == v) ? v : ninf;
            mx = v > mx ? v : mx;
        }
        if (mx > ninf && m_finite(mx)) break;
        st = ST_ERR_WEIGHTS;
    }
    T e[BANK_MAX_HYPOTHESES], d[BANK_MAX_HYPOTHESES];
    T sum = T(0);
#pragma unroll
    for (int j = 0; j < BANK_MAX_HYPOTHESES; ++j) {
        e[j] = T(0);
        d[j] = ninf;
        if (j < Mh) {
            T v = (a.logw_in && pass < 2) ? T(a.logw_in[f0 + j]) : T(0);
            if (a.loglik && pass == 0) v += T(a.loglik[f0 + j]);
            v = (v == v) ? v : ninf;
            d[j] = v - mx;             // <= 0, exactly 0 for the largest
            e[j] = m_exp(d[j]);     // exp(-inf) = 0: a dead hypothesis
            sum += e[j];
        }
    }
    const T ls = m_log(sum), rs = T(1) / sum;
#pragma unroll
    for (int j = 0; j < BANK_MAX_HYPOTHESES; ++j)
        if (j < Mh) {
            a.logw_out[f0 + j] = TS(d[j] - ls);
            if (a.w_out) a.w_out[f0 + j] = TS(e[j] * rs);
        }
    if (a.status) a.status[trk] = st;
}

}  // namespace ukfb
