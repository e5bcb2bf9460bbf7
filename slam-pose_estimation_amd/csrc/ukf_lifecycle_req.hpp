// ukf_lifecycle_req.hpp -- what the lifecycle C-ABI (ukf_lifecycle_api.hip) hands to the kernels of ukf_lifecycle.hpp: the engine's
// per-filter arrays as one untyped argument block, and the pieces of the engine's lifecycle workspace.  No HIP dependency.
#pragma once

#include <stdint.h>

namespace ukfb {

// The engine's per-filter arrays.  Scalars are of the engine's storage type; the kernels cast.
struct LifecycleArrays {
    void* mu = nullptr;            // [cap][S]
    void* cov = nullptr;           // [cap][PK]
    uint32_t* status = nullptr;    // [cap]
    uint8_t* init = nullptr;       // [cap]
    int64_t* last_ts = nullptr;    // [cap]
    void* in_a = nullptr;          // [cap][3] engine-owned latches
    void* in_b = nullptr;
    const void* in_a_read = nullptr;   // what the next prediction reads: the bound buffer if one is bound, else the latch
    const void* in_b_read = nullptr;
    void* Rn = nullptr;            // one D x D matrix, or [cap] of them (noise_per_filter)
    void* Racc = nullptr;          // Pose: the acceleration-branch form of Rn, same count; NULL on OrientationState engines
    const void* acc_cov9 = nullptr;   // Pose: acc.cov in the storage type (the staging buffer of the Racc rebuild)
    int64_t cap = 0;
    int S = 0, PK = 0, D = 0;
    int noise_per_filter = 0;
};

// The engine's lifecycle workspace (ukfb_engine::lifecycle_ws), carved by ukfb::lifecycle_geometry.
struct LifecycleWorkspace {
    uint32_t* owner = nullptr;    // [cap]     scatter: lowest item that names the filter; 0xffffffff (-1 as int32) = free
    uint32_t* counts = nullptr;   // [blocks]  compact: live groups of every count block
    uint32_t* before = nullptr;   // [blocks]  their exclusive prefix sums
    uint32_t* totals = nullptr;   // [4]       L (live groups), H (holes = movers)
    int32_t* hole = nullptr;      // [pair_cap] the pair list: mover[k] is copied onto hole[k]
    int32_t* mover = nullptr;
};

}  // namespace ukfb
