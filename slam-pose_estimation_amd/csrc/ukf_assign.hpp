// ukf_assign.hpp -- ukf_assign_kernel<TS>: the one-to-one assignment of detections to the tracks of a scene
// (include/ukf_batch_assign.h).  One wavefront per scene, ASSIGN_SCENES_PER_GROUP scenes per workgroup, one lane per column of
// the T x (K + T) problem: lanes 0 ... K - 1 are the detections, lane K + t is the private "miss" column of track t, which
// only track t may take.  The algorithm is the shortest augmenting path form of Jonker-Volgenant for rectangular problems
// (Crouse 2016): for each track in order a Dijkstra sweep over the columns until a free column is reached, the dual update,
// and the walk back along `path`.  Every track's miss column is allowed, so every sweep reaches a sink.
//
// Where the state lives: per column (lane j) v, shortest, path, scanned, row4col; per track (lane i) u, col4row, miss.  What a
// step needs of another lane it reads with a wave-uniform lane index (u[i], row4col[j]); only the dual update gathers with a
// per-lane index (shortest[col4row[i]]).  The staged cost block is the one thing in LDS (AssignMap, ukf_host.hpp): doubles,
// +Inf where a pair is forbidden; a step reads row i of it, lane j its element j: only elements the wavefront staged itself
// (i < T, j < K) are ever read.  No workgroup barrier: a wavefront shares nothing with its neighbours.
//
// Every loop has a trip count bounded by a constant: tracks <= 32, steps of a sweep <= ASSIGN_MAX_STEPS (a step scans one
// column), walk back <= ASSIGN_MAX_WALK.  Arithmetic is fp64 for every engine precision (fp32 costs are promoted exactly).
#pragma once

#include <hip/hip_runtime.h>

#include "ukf_host.hpp"

namespace ukfb {

template <class TS> struct AssignArgs {
    const TS* cost;                // [K][cap]
    const TS* miss;                // [cap] or NULL
    const int32_t* scene_start;    // [scenes + 1] or NULL
    int32_t* assign;               // [cap]
    int32_t* owner;                // [scenes][K]
    double* objective;             // [scenes]
    uint32_t* scene_status;        // [scenes]
    double gate, miss_uniform;
    int64_t cap;
    int scenes, K, tracks_per_scene;
};

namespace assign_dev {

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// x of lane `lane`; the index is the same in every lane
__device__ __forceinline__ int read_lane(int x, int lane) { return __builtin_amdgcn_readlane(x, uniform(lane)); }
__device__ __forceinline__ double read_lane(double x, int lane) {
    const int l = uniform(lane);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
// the smallest x of the wavefront, in every lane (x is never NaN here; fmin would drop one)
__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = fmin(x, __shfl_xor(x, m, 64));
    return x;
}
// the sum over the wavefront in a fixed tree order, in every lane
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}
// what the wavefront wrote to LDS is visible to its other lanes behind this point
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace assign_dev

template <class TS> __global__ __launch_bounds__(ASSIGN_THREADS) void ukf_assign_kernel(const AssignArgs<TS> a) {
    using namespace assign_dev;
    constexpr AssignMap map = assign_map();
    __shared__ double lds[map.scalars()];
    const int lane = int(threadIdx.x) & 63, wave = uniform(int(threadIdx.x) >> 6);
    const int s = int(blockIdx.x) * ASSIGN_SCENES_PER_GROUP + wave;
    if (s >= a.scenes) return;
    const double INF = __builtin_huge_val();
    const int K = a.K;

    // the scene's segment, by the rule the host states (assign_segment_ok): a bad scene says so and touches nothing else
    int64_t first, last;
    if (a.scene_start) {
        first = a.scene_start[s];
        last = a.scene_start[s + 1];
    } else {
        assign_uniform_segment(s, a.tracks_per_scene, a.cap, &first, &last);
    }
    if (!assign_segment_ok(first, last, a.cap)) {
        if (lane == 0 && a.scene_status) a.scene_status[s] = UKFB_ASSIGN_BAD_SCENE;
        return;
    }
    const int T = uniform(int(last - first)), ncol = K + T;   // 0 ... 32, <= 64

    // ---- stage: lds[cost(i, k)] = the cost of the pair, +Inf where it is forbidden.  Two candidates per pass, the lanes of a
    // half along the slot index (contiguous in memory)
    {
        const int i = lane & 31, half = lane >> 5;
        for (int k0 = 0; k0 < UKFB_ASSOCIATE_MAX_CANDIDATES; k0 += 2) {
            if (k0 >= K) break;
            const int k = k0 + half;
            if (i < T && k < K) {
                const double c = double(a.cost[int64_t(k) * a.cap + first + i]);
                lds[map.cost(wave, i, k)] = assign_pair_allowed(c, a.gate) ? c : INF;
            }
        }
    }
    // per track (lane i < T): what a miss costs, and whether the track takes part
    double miss = INF;
    if (lane < T) {
        const double m = a.miss ? double(a.miss[first + lane]) : a.miss_uniform;
        if (assign_value_ok(m)) miss = m;
    }
    const unsigned long long eligible = __ballot(lane < T && miss < INF);
    // per column (lane K + t): the cost of track t's miss column
    const double miss_col = __shfl(miss, lane >= K && lane < ncol ? lane - K : 0, 64);
    wave_sync();

    double u = 0.0, v = 0.0;          // duals: u of track `lane`, v of column `lane`
    int col4row = -1, row4col = -1;   // the matching: of track `lane`, of column `lane`
    const double* const block = lds + map.cost(wave, 0, 0);

    for (int cur = 0; cur < UKFB_ASSIGN_MAX_TRACKS; ++cur) {
        if (cur >= T) break;
        if (!((eligible >> cur) & 1ull)) continue;
        // ---- the sweep: shortest reduced distances from track `cur` to the columns, until a free column is scanned
        double shortest = INF, minv = 0.0;
        int path = -1, sink = -1, i = cur;
        bool scanned = false;
        for (int step = 0; step < ASSIGN_MAX_STEPS; ++step) {
            const double ui = read_lane(u, i);
            double c = INF;
            if (lane < K) c = block[i * ASSIGN_ROW_STRIDE + lane];
            else if (lane == K + i) c = miss_col;
            if (!scanned && lane < ncol) {
                const double r = minv + c - ui - v;
                if (r < shortest) {
                    shortest = r;
                    path = i;
                }
            }
            const double key = (!scanned && lane < ncol) ? shortest : INF;
            const double lowest = wave_min(key);
            const unsigned long long at = __ballot(key == lowest);
            if (!(lowest < INF) || at == 0ull) break;   // (no allowed column left: not reached, the miss column is one)
            const int j = uniform(__ffsll(at) - 1);     // ties: the lowest column
            minv = lowest;
            if (lane == j) scanned = true;
            const int r4c = read_lane(row4col, j);
            if (r4c < 0) {
                sink = j;
                break;
            }
            i = r4c;
        }
        if (sink < 0) continue;
        // ---- the dual update: u[cur] += minv; u[i] += minv - shortest[col4row[i]] for the other tracks the sweep visited
        // (those matched to a scanned column); v[j] -= minv - shortest[j] for the scanned columns
        {
            const int cj = col4row >= 0 ? col4row : 0;
            const double sj = __shfl(shortest, cj, 64);
            const int scj = __shfl(int(scanned), cj, 64);
            if (lane == cur) u += minv;
            else if (lane < T && col4row >= 0 && scj) u += minv - sj;
            if (scanned) v -= minv - shortest;
        }
        // ---- the walk back: the sink takes path[sink], that track's former column is handed on, until `cur` is reached
        int j = sink;
        for (int w = 0; w < ASSIGN_MAX_WALK; ++w) {
            const int ti = read_lane(path, j);
            if (ti < 0 || ti >= T) break;   // (not reached: every scanned column has a path)
            if (lane == j) row4col = ti;
            const int prev = read_lane(col4row, ti);
            if (lane == ti) col4row = j;
            if (ti == cur || prev < 0) break;
            j = prev;
        }
    }

    // ---- results.  J in a fixed order: lane i's pair or miss, summed over the wavefront as a tree
    const bool took = lane < T && col4row >= 0 && col4row < K;
    if (a.assign && lane < T) a.assign[first + lane] = took ? col4row : -1;
    if (a.owner && lane < K) a.owner[int64_t(s) * K + lane] = row4col >= 0 ? int32_t(first) + row4col : -1;
    double mine = 0.0;
    if (took) mine = block[lane * ASSIGN_ROW_STRIDE + col4row];
    else if (lane < T && ((eligible >> lane) & 1ull)) mine = miss;
    const double J = wave_sum(mine);
    if (lane == 0) {
        if (a.objective) a.objective[s] = J;
        if (a.scene_status) a.scene_status[s] = UKFB_ASSIGN_OK;
    }
}

}  // namespace ukfb
