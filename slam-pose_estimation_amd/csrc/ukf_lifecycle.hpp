// ukf_lifecycle.hpp -- kernels of the filter lifecycle (include/ukf_batch.h, "filter lifecycle"): gather, scatter, retire, compact.
// Templated on the storage scalar T only; S, PK and D are arguments.
//
// RECORD MOVERS (gather, scatter's write pass, compact's move): one 16-lane row per record, four records per wavefront -- the
// engine's own layout -- and every row issues the loads of its whole record before its first store.  Lane l of a row owns the
// scalars l, l + 16, l + 32, ... of every array, so one instruction of a row covers 16 consecutive scalars (128 B in fp64, 64 B
// in fp32) and the tail of an array is a lane predicate.  The access width is the storage scalar: it is the one width every
// record's stride and start admit (Pose fp64 mu: 104 B, 8-byte aligned; Pose fp32 mu: 52 B and OrientationState fp32 packed
// covariance: 364 B, 4-byte aligned); only Pose fp64 covariances (624 B) would admit 16-byte accesses.
// There is no cross-lane operation in the movers; the block-wide reductions and scans of compact's count / scan / rank kernels
// are called by every thread of their blocks (wave-uniform control flow).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>

#include "../../include/ukf_batch.h"
#include "ukf_host.hpp"
#include "ukf_lifecycle_req.hpp"

namespace ukfb {

// scalars of one array a lane holds at most: ceil(16 / 16) of a mean, ceil(91 / 16) of a packed covariance, ceil(169 / 16) of a noise matrix
constexpr int LC_MU_REGS = 1, LC_COV_REGS = 6, LC_NOISE_REGS = 11;
constexpr uint32_t LC_OWNER_FREE = 0xffffffffu;

// src == nullptr reads zeros; dst == nullptr stores nothing
template <class T, int K> __device__ __forceinline__ void lc_row_load(T (&r)[K], const T* src, int count, int lane) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = lane + LC_ROW * k;
        r[k] = (src && i < count) ? src[i] : T(0);
    }
}
template <class T, int K> __device__ __forceinline__ void lc_row_store(T* dst, const T (&r)[K], int count, int lane) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = lane + LC_ROW * k;
        if (dst && i < count) dst[i] = r[k];
    }
}
template <class T> __device__ __forceinline__ const T* lc_at(const void* base, int64_t record, int stride) {
    return base ? static_cast<const T*>(base) + record * stride : nullptr;
}
template <class T> __device__ __forceinline__ T* lc_at(void* base, int64_t record, int stride) {
    return base ? static_cast<T*>(base) + record * stride : nullptr;
}

// ---- gather: record k <- filter index[k]; read-only on the engine (every engine pointer is read through a pointer to const) ------
template <class T>
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_gather_kernel(const LifecycleArrays a, int64_t n, const int32_t* __restrict__ index,
                                                                          const ukfb_filter_records out) {
    const int64_t k = (int64_t(blockIdx.x) * LC_THREADS + threadIdx.x) / LC_ROW;
    const int lane = int(threadIdx.x) & (LC_ROW - 1);
    if (k >= n) return;
    const int64_t f = index ? int64_t(index[k]) : k;
    const bool valid = f >= 0 && f < a.cap;
    const int S = a.S, PK = a.PK, DD = a.D * a.D;
    T mu[LC_MU_REGS], cov[LC_COV_REGS], nz[LC_NOISE_REGS], ia[1], ib[1];
    lc_row_load(mu, (valid && out.mu) ? lc_at<T>(static_cast<const void*>(a.mu), f, S) : nullptr, S, lane);
    lc_row_load(cov, (valid && out.cov_packed) ? lc_at<T>(static_cast<const void*>(a.cov), f, PK) : nullptr, PK, lane);
    lc_row_load(nz, (valid && out.noise) ? lc_at<T>(static_cast<const void*>(a.Rn), a.noise_per_filter ? f : 0, DD) : nullptr, DD, lane);
    lc_row_load(ia, (valid && out.in_a) ? lc_at<T>(a.in_a_read, f, 3) : nullptr, 3, lane);
    lc_row_load(ib, (valid && out.in_b) ? lc_at<T>(a.in_b_read, f, 3) : nullptr, 3, lane);
    int64_t ts = 0;
    uint8_t flag = 0;
    if (valid && lane == 0) {
        const uint8_t* init = a.init;
        const int64_t* last = a.last_ts;
        flag = init[f];
        ts = last[f];
    }
    lc_row_store(lc_at<T>(out.mu, k, S), mu, S, lane);
    lc_row_store(lc_at<T>(out.cov_packed, k, PK), cov, PK, lane);
    lc_row_store(lc_at<T>(out.noise, k, DD), nz, DD, lane);
    lc_row_store(lc_at<T>(out.in_a, k, 3), ia, 3, lane);
    lc_row_store(lc_at<T>(out.in_b, k, 3), ib, 3, lane);
    if (lane == 0) {
        if (out.initialised) out.initialised[k] = flag;
        if (out.last_ts_us) out.last_ts_us[k] = ts;
        if (out.status) out.status[k] = valid ? 0u : uint32_t(UKFB_ST_INACTIVE);
    }
}

// ---- scatter: the owner pass (lowest item wins), then the write pass ---------------------------------------------------------------
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_claim_kernel(int64_t n, int64_t cap, const int32_t* __restrict__ index, uint32_t* owner) {
    const int64_t k = int64_t(blockIdx.x) * LC_THREADS + threadIdx.x;
    if (k >= n) return;
    const int64_t f = index ? int64_t(index[k]) : k;
    if (f >= 0 && f < cap) atomicMin(&owner[f], uint32_t(k));
}

template <class T>
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_scatter_kernel(const LifecycleArrays a, int64_t n, const int32_t* __restrict__ index,
                                                                           const ukfb_filter_records in, uint32_t* owner) {
    const int64_t k = (int64_t(blockIdx.x) * LC_THREADS + threadIdx.x) / LC_ROW;
    const int lane = int(threadIdx.x) & (LC_ROW - 1);
    if (k >= n) return;
    const int64_t f = index ? int64_t(index[k]) : k;
    const bool valid = f >= 0 && f < a.cap;
    // the winner is the one item for which this holds, whether or not it has released the entry yet
    const bool win = valid && owner[f] == uint32_t(k);
    if (!win) {
        if (lane == 0 && in.status) in.status[k] = uint32_t(UKFB_ST_INACTIVE);
        return;
    }
    const int S = a.S, PK = a.PK, D = a.D, DD = D * D;
    T mu[LC_MU_REGS], cov[LC_COV_REGS], nz[LC_NOISE_REGS], ia[1], ib[1];
    lc_row_load(mu, lc_at<T>(static_cast<const void*>(in.mu), k, S), S, lane);
    lc_row_load(cov, lc_at<T>(static_cast<const void*>(in.cov_packed), k, PK), PK, lane);
    lc_row_load(nz, lc_at<T>(static_cast<const void*>(in.noise), k, DD), DD, lane);
    lc_row_load(ia, lc_at<T>(static_cast<const void*>(in.in_a), k, 3), 3, lane);
    lc_row_load(ib, lc_at<T>(static_cast<const void*>(in.in_b), k, 3), 3, lane);
    uint8_t flag = 1;
    int64_t ts = 0;
    if (lane == 0) {
        if (in.initialised) flag = in.initialised[k] != 0 ? 1 : 0;
        if (in.last_ts_us && flag) ts = in.last_ts_us[k];
    }
    lc_row_store(lc_at<T>(a.mu, f, S), mu, S, lane);
    lc_row_store(lc_at<T>(a.cov, f, PK), cov, PK, lane);
    if (in.in_a) lc_row_store(lc_at<T>(a.in_a, f, 3), ia, 3, lane);
    if (in.in_b) lc_row_store(lc_at<T>(a.in_b, f, 3), ib, 3, lane);
    if (in.noise) {   // (the host has refused noise records on an engine with batch-uniform noise)
        lc_row_store(lc_at<T>(a.Rn, f, DD), nz, DD, lane);
        if (a.Racc) {   // Pose: Rn with block (6,6,3,3) = 2 acc.cov, the expression of build_racc_kernel
            const T* acc9 = static_cast<const T*>(a.acc_cov9);
#pragma unroll
            for (int j = 0; j < LC_NOISE_REGS; ++j) {
                const int i = lane + LC_ROW * j, r = i / D, c = i - r * D;
                if (i < DD && r >= 6 && r < 9 && c >= 6 && c < 9) nz[j] = T(2) * acc9[(r - 6) * 3 + (c - 6)];
            }
            lc_row_store(lc_at<T>(a.Racc, f, DD), nz, DD, lane);
        }
    }
    if (lane == 0) {
        a.init[f] = flag;
        a.last_ts[f] = ts;
        if (in.status) in.status[k] = 0u;
        owner[f] = LC_OWNER_FREE;   // released by its winner: the next call finds the array as the first one did
    }
}

// ---- retire ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_retire_kernel(int64_t cap, const uint8_t* __restrict__ mask, uint8_t* init, int64_t* last_ts) {
    const int64_t i = int64_t(blockIdx.x) * LC_THREADS + threadIdx.x;
    if (i >= cap || !mask[i]) return;
    init[i] = 0;
    last_ts[i] = 0;
}

// ---- compact ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lc_group_live(const uint8_t* __restrict__ init, int64_t g, int group) {
    bool live = false;
    for (int j = 0; j < group; ++j) live = live || init[g * group + j] != 0;
    return live;
}

// counts[b] = live groups among the LC_COUNT_BLOCK groups of block b
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_count_kernel(const uint8_t* __restrict__ init, int64_t G, int group, uint32_t* counts) {
    using Reduce = hipcub::BlockReduce<uint32_t, LC_THREADS>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t base = int64_t(blockIdx.x) * LC_COUNT_BLOCK + int64_t(threadIdx.x) * LC_PER_THREAD;
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < LC_PER_THREAD; ++j)
        if (base + j < G) mine += lc_group_live(init, base + j, group) ? 1u : 0u;
    const uint32_t sum = Reduce(tmp).Sum(mine);
    if (threadIdx.x == 0) counts[blockIdx.x] = sum;
}

// One block: before[b] = live groups of the blocks in front of b, totals[0] = L, totals[1] = H, the dead groups below L.
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_scan_kernel(const uint32_t* __restrict__ counts, int nblocks, const uint8_t* __restrict__ init,
                                                                        int64_t G, int group, uint32_t* before, uint32_t* totals) {
    using Scan = hipcub::BlockScan<uint32_t, LC_THREADS>;
    using Reduce = hipcub::BlockReduce<uint32_t, LC_THREADS>;
    __shared__ typename Scan::TempStorage stmp;
    __shared__ typename Reduce::TempStorage rtmp;
    __shared__ uint32_t below_s;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += LC_THREADS) {
        const int b = b0 + int(threadIdx.x);
        const uint32_t v = b < nblocks ? counts[b] : 0u;
        uint32_t ex, agg;
        Scan(stmp).ExclusiveSum(v, ex, agg);
        if (b < nblocks) before[b] = carry + ex;
        carry += agg;
        __syncthreads();   // the temporary storage is reused, and before[] is read below
    }
    const int64_t L = carry;
    // live groups below L: whole count blocks in front of L's block, and the part of that block below L
    const int64_t bL = L / LC_COUNT_BLOCK;
    const int64_t g0 = bL * LC_COUNT_BLOCK + int64_t(threadIdx.x) * LC_PER_THREAD;
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < LC_PER_THREAD; ++j)
        if (g0 + j < L) mine += lc_group_live(init, g0 + j, group) ? 1u : 0u;
    const uint32_t part = Reduce(rtmp).Sum(mine);
    if (threadIdx.x == 0) {
        const uint32_t front = bL < nblocks ? before[bL] : uint32_t(L);   // (L == G on a block boundary: every group is live)
        totals[0] = uint32_t(L);
        totals[1] = uint32_t(L) - (front + part);
    }
}

// The pair list (hole[k], mover[k]) and the entries of both maps of every filter that stays; the move kernel writes those of the pairs.
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_rank_kernel(const uint8_t* __restrict__ init, int64_t G, int group,
                                                                        const uint32_t* __restrict__ before, const uint32_t* __restrict__ totals,
                                                                        int32_t* hole, int32_t* mover, int64_t pair_cap, int32_t* new_index,
                                                                        int32_t* old_index, int64_t* live_out) {
    using Scan = hipcub::BlockScan<uint32_t, LC_THREADS>;
    __shared__ typename Scan::TempStorage stmp;
    const int64_t L = totals[0], H = totals[1];
    const int64_t base = int64_t(blockIdx.x) * LC_COUNT_BLOCK + int64_t(threadIdx.x) * LC_PER_THREAD;
    bool live[LC_PER_THREAD];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < LC_PER_THREAD; ++j) {
        live[j] = base + j < G && lc_group_live(init, base + j, group);
        mine += live[j] ? 1u : 0u;
    }
    uint32_t ex;
    Scan(stmp).ExclusiveSum(mine, ex);
    int64_t rank = int64_t(before[blockIdx.x]) + ex;   // live groups in front of group base + j
#pragma unroll
    for (int j = 0; j < LC_PER_THREAD; ++j) {
        const int64_t g = base + j;
        if (g >= G) break;
        const bool stays = live[j] && g < L;
        if (!live[j] && g < L) {
            const int64_t k = g - rank;   // dead groups in front of g
            if (k >= 0 && k < pair_cap) hole[k] = int32_t(g);
        } else if (live[j] && g >= L) {
            const int64_t k = rank - (L - H);   // live groups in front of g that are not below L
            if (k >= 0 && k < pair_cap) mover[k] = int32_t(g);
        }
        for (int q = 0; q < group; ++q) {
            const int64_t i = g * group + q;
            // a hole's old index and a mover's new index belong to the move kernel
            if (new_index && (stays || !live[j])) new_index[i] = stays ? int32_t(i) : -1;
            if (old_index && (stays || g >= L)) old_index[i] = stays ? int32_t(i) : -1;
        }
        rank += live[j] ? 1 : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && live_out) *live_out = L * group;
}

// Fixed grid: the rows stride over the totals[1] * group filters to move.  Sources (>= L * group) and destinations (< L * group)
// are disjoint, so there is no staging copy.
template <class T>
__global__ void __launch_bounds__(LC_THREADS) ukf_lifecycle_move_kernel(const LifecycleArrays a, int group, const uint32_t* __restrict__ totals,
                                                                        const int32_t* __restrict__ hole, const int32_t* __restrict__ mover,
                                                                        int32_t* new_index, int32_t* old_index) {
    const int64_t rows = int64_t(gridDim.x) * LC_ROWS_PER_BLOCK;
    const int lane = int(threadIdx.x) & (LC_ROW - 1);
    const int64_t todo = int64_t(totals[1]) * group;
    const int S = a.S, PK = a.PK, DD = a.D * a.D;
    const bool with_noise = a.noise_per_filter != 0;
    for (int64_t t = (int64_t(blockIdx.x) * LC_THREADS + threadIdx.x) / LC_ROW; t < todo; t += rows) {
        const int64_t k = t / group, q = t - k * group;
        const int64_t src = int64_t(mover[k]) * group + q, dst = int64_t(hole[k]) * group + q;
        if (src < 0 || src >= a.cap || dst < 0 || dst >= a.cap) continue;   // (cannot happen: the rank kernel wrote totals[1] pairs)
        T mu[LC_MU_REGS], cov[LC_COV_REGS], nz[LC_NOISE_REGS], na[LC_NOISE_REGS], ia[1], ib[1];
        lc_row_load(mu, lc_at<T>(static_cast<const void*>(a.mu), src, S), S, lane);
        lc_row_load(cov, lc_at<T>(static_cast<const void*>(a.cov), src, PK), PK, lane);
        lc_row_load(ia, lc_at<T>(static_cast<const void*>(a.in_a), src, 3), 3, lane);
        lc_row_load(ib, lc_at<T>(static_cast<const void*>(a.in_b), src, 3), 3, lane);
        lc_row_load(nz, with_noise ? lc_at<T>(static_cast<const void*>(a.Rn), src, DD) : nullptr, DD, lane);
        lc_row_load(na, with_noise ? lc_at<T>(static_cast<const void*>(a.Racc), src, DD) : nullptr, DD, lane);
        uint8_t flag = 0;
        int64_t ts = 0;
        uint32_t st = 0;
        if (lane == 0) {
            flag = a.init[src];
            ts = a.last_ts[src];
            st = a.status[src];
        }
        lc_row_store(lc_at<T>(a.mu, dst, S), mu, S, lane);
        lc_row_store(lc_at<T>(a.cov, dst, PK), cov, PK, lane);
        lc_row_store(lc_at<T>(a.in_a, dst, 3), ia, 3, lane);
        lc_row_store(lc_at<T>(a.in_b, dst, 3), ib, 3, lane);
        if (with_noise) {
            lc_row_store(lc_at<T>(a.Rn, dst, DD), nz, DD, lane);
            lc_row_store(lc_at<T>(a.Racc, dst, DD), na, DD, lane);
        }
        if (lane == 0) {
            a.init[dst] = flag;
            a.last_ts[dst] = ts;
            a.status[dst] = st;
            a.init[src] = 0;
            a.last_ts[src] = 0;
            if (new_index) new_index[src] = int32_t(dst);
            if (old_index) old_index[dst] = int32_t(src);
        }
    }
}

}  // namespace ukfb
