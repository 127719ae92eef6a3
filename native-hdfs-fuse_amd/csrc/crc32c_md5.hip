// crc32c_md5.hip -- batched MD5 over blocks of checksums on the GPU
// (include/hdfs_crc32c.h section 6b): OpBlockChecksumResponseProto.md5
// (datatransfer.proto:262-267) for many HDFS blocks in one launch, from
// checksum arrays that are already in device memory.
//
// MD5 (RFC 1321) is one serial chain per message: 64 dependent steps per 64
// message bytes, nothing to split over lanes.  The unit of parallelism is
// therefore the HDFS block: ONE LANE PER BLOCK, 64 blocks per wave, one wave
// per workgroup (so the waves of a launch spread over the CUs).  A lane walks
// its own checksum array 16 words at a time; the next 16 words are loaded
// before the 64 steps over the current ones begin, so that chain (about 370
// dependent vector instructions) covers the load's latency.  The words after
// the last whole 16 are loaded the same way, each guarded by the lane's word
// count: a lane never reads at or past index n of its array.
//
// Everything that depends on a lane's n is a loop trip count or a guard of
// the tail: lanes with equal n (the blocks of one file) never diverge.
//
// The message is the block's checksums as big-endian bytes; MD5 reads its
// message as little-endian words, so a checksum stored in host order is
// byte-swapped on its way in and one stored in wire order
// (CRC32C_BIG_ENDIAN) is used as it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>

#include "hdfs_crc32c.h"
#include "runtime_internal.h"

namespace hdfs_crc {
namespace {

constexpr uint32_t kMd5ListCap = CRC32C_MD5_LIST_MAX_BLOCKS;
constexpr uint32_t kLanes = 64;  // one wave per workgroup

// Blocks of one contiguous array: block i = sums[i * cpb ...), the last ragged.
struct Md5Contig {
    const uint32_t *sums;
    uint8_t *md5;
    uint64_t nsums;
    uint64_t nblocks;
    uint32_t cpb;
};

// Blocks anywhere: the references ride in the kernel arguments (3 KiB of the
// 4 KiB a launch may carry), nothing is built or uploaded per call.
struct Md5List {
    const uint32_t *sums[kMd5ListCap];
    uint32_t n[kMd5ListCap];
    uint8_t *md5;
    uint32_t nblocks;
};

__device__ constexpr uint32_t kK[64] = {
    0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
    0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
    0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
    0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
    0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
    0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
    0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
    0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
__device__ constexpr uint32_t kS[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};

// The 64 steps of RFC 1321 section 3.4 over one 16-word block (fully
// unrolled: every index and constant is an immediate, the a/b/c/d rotation
// is a renaming).
__device__ __forceinline__ void md5_block(uint32_t (&h)[4], const uint32_t (&m)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        uint32_t f;
        int g;
        if (i < 16) {
            f = d ^ (b & (c ^ d));
            g = i;
        } else if (i < 32) {
            f = c ^ (d & (b ^ c));
            g = (5 * i + 1) & 15;
        } else if (i < 48) {
            f = b ^ c ^ d;
            g = (3 * i + 5) & 15;
        } else {
            f = c ^ (b | ~d);
            g = (7 * i) & 15;
        }
        const uint32_t t = d;
        d = c;
        c = b;
        b = b + __builtin_rotateleft32(a + f + kK[i] + m[g], kS[(i >> 4) * 4 + (i & 3)]);
        a = t;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
}

// Words [16 k, 16 k + 16) of a lane's array as stored: whole while k < full,
// else the `rem` words after the last whole 16 (the rest 0; nothing at or
// past index n = 16 full + rem is read, and nothing at all for rem == 0).
__device__ __forceinline__ void load_words(uint32_t (&w)[16], const uint32_t *src, uint32_t k, uint32_t full,
                                           uint32_t rem) {
    const uint32_t *p = src + size_t(k) * 16;
    if (k < full) {
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = p[j];
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = uint32_t(j) < rem ? p[j] : 0u;
    }
}

template <bool kSwap>
__device__ __forceinline__ void message_words(uint32_t (&m)[16], const uint32_t (&w)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) m[j] = kSwap ? __builtin_bswap32(w[j]) : w[j];
}

// One lane: the MD5 of n checksums at src, its 16 bytes to out (4-byte aligned).
template <bool kSwap>
__device__ __forceinline__ void md5_lane(const uint32_t *src, uint32_t n, uint8_t *out) {
    const uint32_t full = n >> 4, rem = n & 15u;
    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    uint32_t m[16], next[16];
    load_words(next, src, 0, full, rem);
    message_words<kSwap>(m, next);
    for (uint32_t k = 0; k < full; ++k) {
        load_words(next, src, k + 1, full, rem);  // (in flight under the 64 steps below)
        md5_block(h, m);
        message_words<kSwap>(m, next);
    }
    // m: the rem words after the last whole block, then zeros.  Padding (RFC
    // 1321 section 3.1-3.2): a 0x80 byte, zeros to 56 mod 64, the message's
    // length in bits as 64 bits -- in this block when rem <= 13 (a block of
    // its own when rem == 0), else in one more.
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (uint32_t(j) == rem) m[j] = 0x80u;
    const uint32_t finals = rem <= 13 ? 1u : 2u;
    for (uint32_t t = 0; t < finals; ++t) {
        if (t + 1 == finals) {
            m[14] = n << 5;  // 32 n bits, low and high word
            m[15] = n >> 27;
        }
        md5_block(h, m);
#pragma unroll
        for (int j = 0; j < 16; ++j) m[j] = 0;
    }
    uint32_t *o = reinterpret_cast<uint32_t *>(out);  // (little-endian words = RFC byte order)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = h[j];
}

template <bool kSwap>
__global__ __launch_bounds__(kLanes) void hdfs_md5_blocks_kernel(const Md5Contig p) {
    const uint64_t i = uint64_t(blockIdx.x) * kLanes + threadIdx.x;
    if (i >= p.nblocks) return;
    const uint64_t first = i * p.cpb;
    const uint32_t n = uint32_t(std::min<uint64_t>(p.cpb, p.nsums - first));
    md5_lane<kSwap>(p.sums + first, n, p.md5 + 16 * i);
}

template <bool kSwap>
__global__ __launch_bounds__(kLanes) void hdfs_md5_list_kernel(const Md5List p) {
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= p.nblocks) return;
    md5_lane<kSwap>(p.sums[i], p.n[i], p.md5 + 16 * size_t(i));
}

int check_common(const crc32c_ctx *ctx, uint32_t flags, const uint8_t *dev_md5) {
    if (!ctx) return fail(-EINVAL, "ctx == NULL");
    if (flags & ~CRC32C_BIG_ENDIAN) return fail(-EINVAL, "block MD5 takes only CRC32C_BIG_ENDIAN (flags 0x%x)", flags);
    if (!dev_md5) return fail(-EINVAL, "dev_md5 == NULL");
    if (uintptr_t(dev_md5) & 3u) return fail(-EINVAL, "dev_md5 is not 4-byte aligned");
    return 0;
}

// The list launches of (dev_sums[i], nsums[i]) -> dev_md5 + 16 i; the
// arguments are checked already.
int launch_list(const crc32c_ctx *ctx, const uint32_t *const *dev_sums, const uint32_t *nsums, uint32_t same_n,
                size_t nblocks, uint32_t flags, uint8_t *dev_md5, hipStream_t s) {
    DeviceGuard guard(ctx->device);
    Md5List p;
    for (size_t i = 0; i < nblocks; i += kMd5ListCap) {
        const uint32_t c = uint32_t(std::min<size_t>(kMd5ListCap, nblocks - i));
        for (uint32_t k = 0; k < c; ++k) {
            p.sums[k] = dev_sums[i + k];
            p.n[k] = nsums ? nsums[i + k] : same_n;
        }
        p.md5 = dev_md5 + 16 * i;
        p.nblocks = c;
        const dim3 g{(c + kLanes - 1) / kLanes, 1, 1}, b{kLanes, 1, 1};
        if (flags & CRC32C_BIG_ENDIAN)
            hipLaunchKernelGGL(hdfs_md5_list_kernel<false>, g, b, 0, s, p);
        else
            hipLaunchKernelGGL(hdfs_md5_list_kernel<true>, g, b, 0, s, p);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

// Loads this file's code object onto the current device (crc32c_ctx_create,
// beside preload_plan_kernels: a process's first MD5 call then does not pay
// the load).
hipError_t preload_md5_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&hdfs_md5_blocks_kernel<true>));
}

}  // namespace hdfs_crc

using namespace hdfs_crc;

extern "C" {

int crc32c_md5_blocks(crc32c_ctx *ctx, const uint32_t *dev_sums, uint64_t nsums, uint32_t crc_per_block,
                      uint32_t flags, uint8_t *dev_md5, void *stream) {
    if (int rc = check_common(ctx, flags, dev_md5)) return rc;
    if (nsums == 0) return 0;
    if (crc_per_block == 0) return fail(-EINVAL, "crc_per_block == 0");
    if (!dev_sums) return fail(-EINVAL, "dev_sums == NULL");
    if (uintptr_t(dev_sums) & 3u) return fail(-EINVAL, "dev_sums is not 4-byte aligned");
    Md5Contig p;
    p.sums = dev_sums;
    p.md5 = dev_md5;
    p.nsums = nsums;
    p.nblocks = crc32c_md5_nblocks(nsums, crc_per_block);
    p.cpb = crc_per_block;
    const uint64_t grid = (p.nblocks + kLanes - 1) / kLanes;
    if (grid > 0x7fffffffull) return fail(-EINVAL, "%llu blocks are more than one launch holds", (unsigned long long)p.nblocks);
    DeviceGuard guard(ctx->device);
    const dim3 g{uint32_t(grid), 1, 1}, b{kLanes, 1, 1};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & CRC32C_BIG_ENDIAN)
        hipLaunchKernelGGL(hdfs_md5_blocks_kernel<false>, g, b, 0, s, p);
    else
        hipLaunchKernelGGL(hdfs_md5_blocks_kernel<true>, g, b, 0, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

int crc32c_md5_block_list(crc32c_ctx *ctx, const uint32_t *const *dev_sums, const uint32_t *nsums, size_t nblocks,
                          uint32_t flags, uint8_t *dev_md5, void *stream) {
    if (int rc = check_common(ctx, flags, dev_md5)) return rc;
    if (nblocks == 0) return 0;
    if (!dev_sums || !nsums) return fail(-EINVAL, "dev_sums/nsums == NULL");
    for (size_t i = 0; i < nblocks; ++i) {
        if (nsums[i] && !dev_sums[i]) return fail(-EINVAL, "block %zu: %u checksums at NULL", i, nsums[i]);
        if (uintptr_t(dev_sums[i]) & 3u) return fail(-EINVAL, "block %zu: checksums not 4-byte aligned", i);
    }
    return launch_list(ctx, dev_sums, nsums, 0, nblocks, flags, dev_md5, static_cast<hipStream_t>(stream));
}

int crc32c_plan_exec_blocks_md5(crc32c_plan *plan, const void *const *dev_payloads, uint32_t *const *dev_outs,
                                size_t nblocks, uint8_t *dev_md5, void *stream) {
    if (!plan) return fail(-EINVAL, "plan == NULL");
    if (int rc = check_common(plan->ctx, plan->flags & CRC32C_BIG_ENDIAN, dev_md5)) return rc;
    if (plan->nchecksums > UINT32_MAX) return fail(-EINVAL, "a block of more than 2^32 - 1 checksums");
    if (nblocks == 0) return 0;
    if (!dev_payloads || !dev_outs) return fail(-EINVAL, "payloads/outs == NULL");
    for (size_t i = 0; i < nblocks; ++i)
        if (!dev_outs[i] || (uintptr_t(dev_outs[i]) & 3u))
            return fail(-EINVAL, "block %zu: out NULL / not 4-byte aligned", i);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    // (exec_blocks checks the rest before it launches anything)
    if (int rc = exec_blocks(plan, dev_payloads, dev_outs, nblocks, s, nullptr)) return rc;
    return launch_list(plan->ctx, dev_outs, nullptr, uint32_t(plan->nchecksums), nblocks,
                       plan->flags & CRC32C_BIG_ENDIAN, dev_md5, s);
}

}  // extern "C"
