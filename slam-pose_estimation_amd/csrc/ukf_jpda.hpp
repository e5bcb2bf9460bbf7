// ukf_jpda.hpp -- ukf_jpda_kernel<TS>: the exact joint association marginals of a scene (include/ukf_batch_jpda.h,
// DESIGN.md 4.32).  One wavefront per scene, JPDA_SCENES_PER_GROUP scenes per workgroup, one lane per SUBSET S of the
// scene's tracks: the lane index is the subset's bitmask (T <= 6 tracks, 2^6 = 64 lanes).  With the detections taken in order,
//   F_k[S] = the weight of the matchings of detections 0 ... k - 1 onto exactly the tracks in S,
//            F_{k+1}[S] = F_k[S] + sum_{i in S} psi_ik F_k[S xor 2^i],                       F_0 = [S is empty];
//   G_k[U] = the weight of the matchings of detections k ... K - 1 onto tracks outside U,
//            G_k[U] = G_{k+1}[U] + sum_{i not in U} psi_ik G_{k+1}[U xor 2^i],               G_K = 1;  Z = G_0[empty];
//   beta_ik = sum_{S without i} F_k[S] psi_ik G_{k+1}[S xor 2^i] / Z,   beta_i0 = sum_{S without i} F_K[S] / Z.
// Removing a track from a subset, or adding one, is an xor on the lane index: a step is T cross-lane xor exchanges and T fma,
// and there is no per-lane gather index anywhere.  Every sum has positive terms only.
//
// Where the state lives: psi is staged ONCE into registers, lane k holding psi_ik for the six tracks i, and a step reads it with
// a constant lane index (the detection loops are unrolled to the constant 32 under wave-uniform guards); the backward table
// G_1 ... G_32 lives in 32 fp64 registers (G_{k+1} = 1 beyond K); F is one register.  The backward pass runs first, so Z is
// known when the forward pass forms each beta_ik and stores it.  No LDS, no workgroup barrier: a wavefront shares nothing with
// its neighbours, and its result does not depend on its position in the workgroup.
//
// Every loop has a constant bound: a `for` over the tracks (<= 6), and the detection loops (<= 32) written as the compile-time
// recursion each_detection, because their unrolled bodies exceed what `#pragma unroll` will expand and a loop left rolled
// would index the register table dynamically, that is, move it to scratch.  Arithmetic is fp64 for every engine precision
// (fp32 inputs are promoted exactly).  Lanes of subsets that name a track >= T hold F = 0 and a finite G: they add exact zeros.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "ukf_host.hpp"

namespace ukfb {

template <class TS> struct JpdaArgs {
    const TS* loglik;              // [K][cap]
    const TS* maha;                // [K][cap] or NULL
    const int32_t* model;          // [cap] or NULL
    const int32_t* scene_start;    // [scenes + 1] or NULL
    TS* beta;                      // [K][cap]
    TS* beta0;                     // [cap]
    double* free_k;                // [scenes][K]
    double* log_z;                 // [scenes]
    uint32_t* scene_status;        // [scenes]
    double gate, ln_pd, a0_m1, a0_m3;
    int64_t cap;
    int scenes, K, tracks_per_scene, model_uniform, engine_model;
};

namespace jpda_dev {

constexpr int TMAX = UKFB_JPDA_MAX_TRACKS, KMAX = UKFB_ASSOCIATE_MAX_CANDIDATES;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// x of lane `lane`, a constant of the unrolled loop
__device__ __forceinline__ double read_lane(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane), __builtin_amdgcn_readlane(__double2loint(x), lane));
}
// the sum over the wavefront in a fixed tree order, in every lane
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// f(k) for k = 0 ... KMAX - 1 with k a constant of each call
template <int B = 0, class F> __device__ __forceinline__ void each_detection(F&& f) {
    if constexpr (B < KMAX) {
        f(std::integral_constant<int, B>{});
        each_detection<B + 1>(f);
    }
}

}  // namespace jpda_dev

template <class TS> __global__ __launch_bounds__(JPDA_THREADS) void ukf_jpda_kernel(const JpdaArgs<TS> a) {
    using namespace jpda_dev;
    const int lane = int(threadIdx.x) & 63, wave = uniform(int(threadIdx.x) >> 6);
    const int s = int(blockIdx.x) * JPDA_SCENES_PER_GROUP + wave;
    if (s >= a.scenes) return;
    const int K = a.K;

    // the scene's segment, by the rule the host states (jpda_segment_status): a bad or too-large scene says so and touches
    // nothing else
    int64_t first, last;
    if (a.scene_start) {
        first = a.scene_start[s];
        last = a.scene_start[s + 1];
    } else {
        assign_uniform_segment(s, a.tracks_per_scene, a.cap, &first, &last);
    }
    const uint32_t verdict = jpda_segment_status(first, last, a.cap);
    if (verdict != UKFB_JPDA_OK) {
        if (lane == 0 && a.scene_status) a.scene_status[s] = verdict;
        return;
    }
    const int T = uniform(int(last - first));   // 0 ... 6

    // ---- stage psi once: lane k holds psi_ik of the tracks i < T; bit i of `scored`: loglik of (i, k) is finite
    double psi[TMAX];
    uint32_t scored = 0u;
#pragma unroll
    for (int i = 0; i < TMAX; ++i) {
        psi[i] = 0.0;
        if (i < T) {
            const int mid = a.model ? a.model[first + i] : a.model_uniform;
            const double a0 = jpda_kernel_dim(a.engine_model, int64_t(mid)) == 1 ? a.a0_m1 : a.a0_m3;
            if (lane < K) {
                const int64_t at = int64_t(lane) * a.cap + first + i;
                const double ll = double(a.loglik[at]);
                const double d2 = a.maha ? double(a.maha[at]) : 0.0;
                const double l = (a.ln_pd + ll) - a0;
                if (jpda_finite(ll)) scored |= 1u << i;
                if (jpda_pair_allowed(ll, d2, a.gate)) psi[i] = exp(fmin(l, double(UKFB_JPDA_LOG_RATIO_MAX)));
            }
        }
    }

    // ---- backward: Gs[k] = G_{k+1}, from G_K = 1 down; Z = G_0 of the empty set (lane 0)
    double Gs[KMAX];
    double g = 1.0;
    each_detection([&](auto kk) {
        constexpr int k = KMAX - 1 - decltype(kk)::value;
        Gs[k] = g;
        if (k < K) {
            double acc = g;
#pragma unroll
            for (int i = 0; i < TMAX; ++i) {
                if (i < T) {
                    const double p = read_lane(psi[i], k);
                    const double x = __shfl_xor(g, 1 << i, 64);
                    acc = ((lane >> i) & 1) ? acc : fma(p, x, acc);
                }
            }
            g = acc;
        }
    });
    const double Z = read_lane(g, 0);
    const double rz = 1.0 / Z;   // (Z >= 1: the all-miss event)

    // ---- forward: F_k, and per detection the marginals beta_ik (lane i keeps its track's), stored as a row of T values
    const double nanv = __builtin_nan("");
    double f = lane == 0 ? 1.0 : 0.0;
    each_detection([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if (k < K) {
            const double g1 = Gs[k];
            double nf = f, mine = 0.0, taken = 0.0;
#pragma unroll
            for (int i = 0; i < TMAX; ++i) {
                if (i < T) {
                    const bool has = ((lane >> i) & 1) != 0;
                    const double p = read_lane(psi[i], k);
                    const double t = p * __shfl_xor(g1, 1 << i, 64);    // the term the backward step formed
                    const double b = wave_sum(has ? 0.0 : f * t) * rz;
                    mine = (lane == i) ? b : mine;
                    taken += b;
                    const double x = __shfl_xor(f, 1 << i, 64);
                    nf = has ? fma(p, x, nf) : nf;
                }
            }
            f = nf;
            const uint32_t sc = uint32_t(__builtin_amdgcn_readlane(int(scored), k));
            if (a.beta && lane < T) a.beta[int64_t(k) * a.cap + first + lane] = TS(((sc >> lane) & 1u) ? mine : nanv);
            if (a.free_k && lane == 0) a.free_k[int64_t(s) * K + k] = 1.0 - taken;
        }
    });
    // ---- beta_i0 = sum over the subsets without i of F_K / Z
    {
        double mine = 0.0;
#pragma unroll
        for (int i = 0; i < TMAX; ++i) {
            if (i < T) {
                const double b = wave_sum(((lane >> i) & 1) ? 0.0 : f) * rz;
                mine = (lane == i) ? b : mine;
            }
        }
        if (a.beta0 && lane < T) a.beta0[first + lane] = TS(mine);
    }
    if (lane == 0) {
        if (a.log_z) a.log_z[s] = log(Z);
        if (a.scene_status) a.scene_status[s] = UKFB_JPDA_OK;
    }
}

}  // namespace ukfb
