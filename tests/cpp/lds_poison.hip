// Test helper: fills the LDS of every CU with a bit pattern (NaN, Inf, zero) so that a following kernel finds those
// leftovers wherever it has not written itself.  tests/test_gpu_lds_leftovers.py runs the engine after different patterns
// and demands identical results: no kernel may depend on LDS it did not initialise (round 3: a pad scalar between two LDS
// regions was read as "garbage times exact zero", which is NaN when the garbage is).
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ void lds_fill_kernel(uint32_t pattern, int dwords, uint32_t* sink) {
    extern __shared__ uint32_t lds[];
    for (int i = threadIdx.x; i < dwords; i += blockDim.x) lds[i] = pattern;
    __syncthreads();
    // read something back so that the stores cannot be dropped
    if (threadIdx.x == 0 && lds[(blockIdx.x * 131) % dwords] != pattern) sink[0] = 1u;
}

// The canary of the instrument: the fill's geometry, no LDS store, every dword of the workgroup's own allocation read and
// compared with the pattern.  The volatile reads cannot be folded into "uninitialised, any value will do".
__global__ void lds_seen_kernel(uint32_t pattern, int dwords, unsigned long long* counts) {
    extern __shared__ uint32_t lds[];
    const volatile uint32_t* p = lds;
    unsigned long long matched = 0, read = 0;
    for (int i = threadIdx.x; i < dwords; i += blockDim.x) {
        matched += p[i] == pattern ? 1u : 0u;
        read += 1u;
    }
    atomicAdd(&counts[0], matched);
    atomicAdd(&counts[1], read);
}

// matched = the dwords that still held `pattern`, read = the dwords looked at (grid x 160 KiB / 4); returns 0
extern "C" int lds_leftovers_seen(uint32_t pattern, uint64_t* matched, uint64_t* read) {
    const int bytes = 160 * 1024;
    if (matched == nullptr || read == nullptr) return 4;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(lds_seen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return 1;
    unsigned long long* counts = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&counts), 16) != hipSuccess) return 2;
    unsigned long long host[2] = {0, 0};
    hipError_t err = hipMemset(counts, 0, 16);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(lds_seen_kernel, dim3(256 * 4), dim3(256), bytes, 0, pattern, bytes / 4, counts);
        err = hipDeviceSynchronize();
    }
    if (err == hipSuccess) err = hipMemcpy(host, counts, 16, hipMemcpyDeviceToHost);
    (void)hipFree(counts);
    *matched = host[0];
    *read = host[1];
    return err == hipSuccess ? 0 : 3;
}

extern "C" int lds_poison(uint32_t pattern) {
    const int bytes = 160 * 1024;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(lds_fill_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return 1;
    uint32_t* sink = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&sink), 4) != hipSuccess) return 2;
    (void)hipMemset(sink, 0, 4);
    // one workgroup owns the whole LDS of a CU; several per CU in turn so that every CU is visited
    hipLaunchKernelGGL(lds_fill_kernel, dim3(256 * 4), dim3(256), bytes, 0, pattern, bytes / 4, sink);
    const hipError_t err = hipDeviceSynchronize();
    (void)hipFree(sink);
    return err == hipSuccess ? 0 : 3;
}
