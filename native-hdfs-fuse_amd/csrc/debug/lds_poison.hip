// lds_poison.hip -- fills every CU's LDS with a known non-table pattern, and
// counts how much of it a later launch still finds (debug library only).
//
// LDS is not cleared between launches: a kernel build that stages too little
// of its table image still reads the tables the launch before it left there.
// A test that poisons the LDS right before each launch on the same stream
// makes such a build read the pattern instead (tests/test_gpu_cold_lds.py;
// the control there, kernel variant 96, stages nothing and must come out
// wrong).  Each workgroup takes the CU's whole LDS (160 KiB), so one fits per
// CU and 4 x CUs of them cover an idle chip.
#include <hip/hip_runtime.h>

#include <cerrno>

#include "../runtime_internal.h"
#include "hdfs_crc32c_debug.h"

namespace {

constexpr uint32_t kLdsWords = 163840 / 4;  // the whole LDS of a gfx950 CU
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWgPerCu = 4;

// (the LDS address space, so that the accesses are ds instructions, not flat ones)
typedef volatile __attribute__((address_space(3))) uint32_t *LdsWords;

__device__ inline uint32_t pattern(uint32_t seed, uint32_t i) { return (seed ^ (i * 0x9E3779B9u)) | 1u; }

// (volatile: the stores have no reader in this kernel and stay anyway)
__global__ __launch_bounds__(kThreads) void lds_poison_kernel(uint32_t seed) {
    __shared__ uint32_t lds[kLdsWords];
    LdsWords v = (LdsWords)lds;
    for (uint32_t i = threadIdx.x; i < kLdsWords; i += kThreads) v[i] = pattern(seed, i);
}

// counts[workgroup] += words still holding the pattern (counts zeroed by the
// caller).  `never` is always 0: a possible store keeps the compiler from
// treating the never-written array as undefined and dropping the reads.
__global__ __launch_bounds__(kThreads) void lds_peek_kernel(uint32_t seed, uint32_t never, uint32_t *counts) {
    __shared__ uint32_t lds[kLdsWords];
    LdsWords v = (LdsWords)lds;
    if (never) v[threadIdx.x] = seed;
    uint32_t n = 0;
    for (uint32_t i = threadIdx.x; i < kLdsWords; i += kThreads) n += v[i] == pattern(seed, i) ? 1u : 0u;
    if (n) atomicAdd(counts + blockIdx.x, n);
}

// Workgroups of a poison / peek launch on the current device, or -errno.
int poison_grid() {
    using namespace hdfs_crc;
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus <= 0) return fail(-ENODEV, "no compute units");
    return int(kWgPerCu) * cus;
}

}  // namespace

extern "C" int crc32c_debug_lds_poison(uint32_t seed, void *stream) {
    using namespace hdfs_crc;
    const int grid = poison_grid();
    if (grid < 0) return grid;
    hipLaunchKernelGGL(lds_poison_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       seed);
    HIP_TRY(hipGetLastError());
    return grid;
}

extern "C" int crc32c_debug_lds_peek(uint32_t seed, uint32_t *dev_counts, void *stream) {
    using namespace hdfs_crc;
    const int grid = poison_grid();
    if (grid < 0 || !dev_counts) return grid;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(dev_counts, 0, size_t(grid) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(lds_peek_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, s, seed, 0u, dev_counts);
    HIP_TRY(hipGetLastError());
    return grid;
}
