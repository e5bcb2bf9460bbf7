// ukf_buckets.hip -- the model-class buckets of ukfb_cycle_dev with per-filter model ids: the kernels that group the filter
// indices by the class of their update, build_model_buckets, and ukfb_last_model_groups.  Its kernels use hipCUB's block-wide
// reduce and scan alone (the two block headers, not the whole library).
#include "ukf_api_common.hpp"   // first: hipCUB's block headers pick their backend from what the HIP runtime header defines

#include <hipcub/block/block_reduce.hpp>
#include <hipcub/block/block_scan.hpp>

using namespace ukfb;

namespace {
// ---- model-class buckets (ukfb_cycle_dev with per-filter model ids) ---------------------------------------
// A stable three-way partition (by update_class above) of the filter indices, two passes over the model ids: (1) per-block class
// counts, (2) ONE block turns them into exclusive prefix sums and class totals (3 x blocks values: 120 000 at the 40-million-
// filter capacity the tests exercise; every scatter block re-summing all of them was quadratic in the batch size), (3) every
// block scatters from its offsets.  The
// classes follow each other from the most expensive to the cheapest, each
// starts at a multiple of 4 (one wavefront = 4 filters); the gaps behind the classes are filled with -1 (padding) by the scatter kernel.
using ukfb::BK_THREADS, ukfb::BK_PER_THREAD, ukfb::BK_BLOCK;
__global__ void __launch_bounds__(BK_THREADS) bucket_count_kernel(const int32_t* meas, int64_t n, int engine_model, uint32_t* counts,
                                                                  int nblocks) {
    using Reduce = hipcub::BlockReduce<uint32_t, BK_THREADS>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t base = int64_t(blockIdx.x) * BK_BLOCK + int64_t(threadIdx.x) * BK_PER_THREAD;
    uint32_t c1 = 0, c2 = 0, valid = 0;
#pragma unroll
    for (int j = 0; j < BK_PER_THREAD; ++j)
        if (base + j < n) {
            const int c = ukfb::update_class(engine_model, meas[base + j]);
            c1 += c == 1;
            c2 += c == 2;
            ++valid;
        }
    // (counts of at most 1024 each: two of them share a word)
    const uint32_t packed = Reduce(tmp).Sum(c1 | (c2 << 16));
    __syncthreads();
    const uint32_t tot = Reduce(tmp).Sum(valid);
    if (threadIdx.x == 0) {
        const uint32_t n1 = packed & 0xFFFFu, n2 = packed >> 16;
        counts[blockIdx.x] = tot - n1 - n2;
        counts[nblocks + blockIdx.x] = n1;
        counts[2 * nblocks + blockIdx.x] = n2;
    }
}
// exclusive prefix sums of the per-block counts, class by class: before[c * nblocks + b] = sum of counts[c][0 .. b), total[c]
constexpr int BS_THREADS = 1024;
__global__ void __launch_bounds__(BS_THREADS) bucket_scan_kernel(const uint32_t* counts, int nblocks, uint32_t* before, uint32_t* total) {
    using Scan = hipcub::BlockScan<uint32_t, BS_THREADS>;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ uint32_t carry;
    for (int c = 0; c < 3; ++c) {
        if (threadIdx.x == 0) carry = 0;
        __syncthreads();
        for (int b0 = 0; b0 < nblocks; b0 += BS_THREADS) {
            const int b = b0 + int(threadIdx.x);
            const uint32_t v = b < nblocks ? counts[c * nblocks + b] : 0u;
            uint32_t ex, tile;
            Scan(tmp).ExclusiveSum(v, ex, tile);
            if (b < nblocks) before[c * nblocks + b] = carry + ex;
            __syncthreads();
            if (threadIdx.x == 0) carry += tile;
            __syncthreads();
        }
        if (threadIdx.x == 0) total[c] = carry;
        __syncthreads();
    }
}
// INLINE_SCAN (launches of up to BUCKET_INLINE_BLOCKS blocks): every block sums the per-block counts itself -- its own exclusive
// prefix and the class totals, 3 x nblocks values -- instead of reading them from bucket_scan_kernel's output: one launch fewer
// where the launches, not the sums, are what the grouping costs (four launches of ~5 us each per cycle at 262 144 filters were 6.6 %
// of config 5's cycle).  Block 0 also writes the padding (-1) behind each class and up to `items`: no memset of the list.
template <bool INLINE_SCAN>
__global__ void __launch_bounds__(BK_THREADS) bucket_scatter_kernel(const int32_t* meas, int64_t n, int engine_model, const uint32_t* counts,
                                                                    const uint32_t* before, const uint32_t* total, int nblocks,
                                                                    int32_t* order, uint32_t items) {
    using Scan = hipcub::BlockScan<uint32_t, BK_THREADS>;
    using Reduce64 = hipcub::BlockReduce<unsigned long long, BK_THREADS>;
    __shared__ typename Scan::TempStorage stmp;
    __shared__ typename Reduce64::TempStorage rtmp;
    __shared__ uint32_t start[3];
    if constexpr (INLINE_SCAN) {
        __shared__ uint32_t pre_s[3], tot_s[3];
        for (int c = 0; c < 3; ++c) {
            unsigned long long acc = 0;   // low word: counts of the blocks before this one, high word: of all blocks
            for (int b = int(threadIdx.x); b < nblocks; b += BK_THREADS) {
                const unsigned long long v = counts[c * nblocks + b];
                acc += (v << 32) | (b < int(blockIdx.x) ? v : 0ull);
            }
            const unsigned long long sum = Reduce64(rtmp).Sum(acc);
            if (threadIdx.x == 0) {
                pre_s[c] = uint32_t(sum);
                tot_s[c] = uint32_t(sum >> 32);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const uint32_t b1 = (tot_s[2] + 3u) & ~3u, b0 = b1 + ((tot_s[1] + 3u) & ~3u);
            start[2] = pre_s[2];
            start[1] = b1 + pre_s[1];
            start[0] = b0 + pre_s[0];
        }
        if (blockIdx.x == 0 && threadIdx.x < 16) {   // the gaps behind the three classes (at most 3 + 3 + 12 entries)
            const uint32_t b1 = (tot_s[2] + 3u) & ~3u, b0 = b1 + ((tot_s[1] + 3u) & ~3u);
            const uint32_t t = threadIdx.x;
            if (tot_s[2] + t < b1) order[tot_s[2] + t] = -1;
            if (b1 + tot_s[1] + t < b0) order[b1 + tot_s[1] + t] = -1;
            if (b0 + tot_s[0] + t < items) order[b0 + tot_s[0] + t] = -1;
        }
    } else {
        if (threadIdx.x == 0) {
            // the most expensive class first: the cheap wavefronts fill the tail of the launch
            const uint32_t b1 = (total[2] + 3u) & ~3u, b0 = b1 + ((total[1] + 3u) & ~3u);
            start[2] = before[2 * nblocks + blockIdx.x];
            start[1] = b1 + before[nblocks + blockIdx.x];
            start[0] = b0 + before[blockIdx.x];
        }
        if (blockIdx.x == 0 && threadIdx.x < 16) {
            const uint32_t b1 = (total[2] + 3u) & ~3u, b0 = b1 + ((total[1] + 3u) & ~3u);
            const uint32_t t = threadIdx.x;
            if (total[2] + t < b1) order[total[2] + t] = -1;
            if (b1 + total[1] + t < b0) order[b1 + total[1] + t] = -1;
            if (b0 + total[0] + t < items) order[b0 + total[0] + t] = -1;
        }
    }
    __syncthreads();
    const int64_t base = int64_t(blockIdx.x) * BK_BLOCK + int64_t(threadIdx.x) * BK_PER_THREAD;
    int cls[BK_PER_THREAD];
#pragma unroll
    for (int j = 0; j < BK_PER_THREAD; ++j) cls[j] = (base + j < n) ? ukfb::update_class(engine_model, meas[base + j]) : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < BK_PER_THREAD; ++j) mine += cls[j] == c;
        uint32_t rank;
        Scan(stmp).ExclusiveSum(mine, rank);
        __syncthreads();
        rank += start[c];
#pragma unroll
        for (int j = 0; j < BK_PER_THREAD; ++j)
            if (cls[j] == c) order[rank++] = int32_t(base + j);
    }
}
}  // namespace

namespace ukfb {
// fills e->bucket_idx for the model ids in meas_dev; *items = entries of the list that a launch must cover (an upper bound
// known without reading anything back: every class is padded to a multiple of 4)
int build_model_buckets(ukfb_engine* e, const int32_t* meas_dev, int64_t* items) {
    const int64_t n = e->cap;
    const ukfb::BucketGeometry geo = ukfb::bucket_geometry(n);
    const int nblocks = geo.blocks;
    if (!e->bucket_idx || !e->bucket_counts) {
        // both or neither: the engine sees the pair only when every allocation succeeded (a half-published pair would let the
        // next call skip the allocation and launch through a null pointer)
        int32_t* idx = nullptr;
        uint32_t* cnt = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&idx), geo.list * sizeof(int32_t)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&cnt), geo.count_words * sizeof(uint32_t)) != hipSuccess) {
            if (idx) (void)hipFree(idx);
            return fail(UKFB_ERR_HIP, "model buckets: device allocation failed");
        }
        if (e->bucket_idx) (void)hipFree(e->bucket_idx);
        if (e->bucket_counts) (void)hipFree(e->bucket_counts);
        e->bucket_idx = idx;
        e->bucket_counts = cnt;
    }
    uint32_t* const before = e->bucket_counts + size_t(3) * nblocks;
    uint32_t* const total = e->bucket_counts + size_t(6) * nblocks;
    *items = geo.items;
    // (the gaps of the list -- behind each class, up to *items -- are written by the scatter kernel: no memset)
    hipLaunchKernelGGL(bucket_count_kernel, dim3(nblocks), dim3(BK_THREADS), 0, ukfb::main_stream(e), meas_dev, n, e->model, e->bucket_counts,
                       nblocks);
    if (geo.inline_scan) {
        hipLaunchKernelGGL(bucket_scatter_kernel<true>, dim3(nblocks), dim3(BK_THREADS), 0, ukfb::main_stream(e), meas_dev, n, e->model,
                           static_cast<const uint32_t*>(e->bucket_counts), static_cast<const uint32_t*>(before),
                           static_cast<const uint32_t*>(total), nblocks, e->bucket_idx, uint32_t(*items));
    } else {
        hipLaunchKernelGGL(bucket_scan_kernel, dim3(1), dim3(BS_THREADS), 0, ukfb::main_stream(e),
                           static_cast<const uint32_t*>(e->bucket_counts), nblocks, before, total);
        hipLaunchKernelGGL(bucket_scatter_kernel<false>, dim3(nblocks), dim3(BK_THREADS), 0, ukfb::main_stream(e), meas_dev, n, e->model,
                           static_cast<const uint32_t*>(e->bucket_counts), static_cast<const uint32_t*>(before),
                           static_cast<const uint32_t*>(total), nblocks, e->bucket_idx, uint32_t(*items));
    }
    HIP_TRY(hipGetLastError());
    e->bucket_items = *items;
    return UKFB_OK;
}
}  // namespace ukfb

extern "C" {

int ukfb_last_model_groups(ukfb_engine* e, int32_t* list, int64_t capacity, int64_t* items) {
    if (!e || !items || (capacity > 0 && !list)) return UKFB_ERR_INVALID_ARG;
    ON_DEVICE(e->device);
    *items = e->bucket_items;
    if (!e->bucket_idx || e->bucket_items == 0) return fail(UKFB_ERR_INVALID_ARG, "no launch of this engine has grouped its filters by update class");
    const int64_t n = capacity < e->bucket_items ? capacity : e->bucket_items;
    if (n > 0) {
        HIP_TRY(hipStreamSynchronize(ukfb::main_stream(e)));
        HIP_TRY(hipMemcpy(list, e->bucket_idx, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return UKFB_OK;
}

}  // extern "C"
