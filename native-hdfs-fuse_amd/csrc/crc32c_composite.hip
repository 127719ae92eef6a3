// crc32c_composite.hip -- composite CRCs on the GPU (include/hdfs_crc32c.h
// section 6c): the chunk checksums of a cell (an HDFS block, or a stripe cell)
// combined into the CRC of the cell's bytes, for many cells per launch, from
// checksum arrays that are already in device memory.
//
// The algebra ("composite CRC"): with X = x^(8 bpc) in
// GF(2)[x] mod P, a cell of checksums c_0 .. c_{n-1} whose last chunk is L
// bytes long has the CRC
//     H x^(8 L) ^ c_{n-1},   H = c_0 X^(m-1) ^ c_1 X^(m-2) ^ ... ^ c_{m-1},  m = n - 1.
// H is a sum of weighted terms, so it is cut into SEGMENTS of kSeg = 8192
// terms counted from the right (segment r holds the terms whose weights are
// X^(r kSeg) .. X^((r + 1) kSeg - 1); the leftmost one is ragged), and
//
//  * ONE WAVE PER SEGMENT.  The segment is right-aligned in a grid of kRun
//    rows of 64 lanes (missing leading terms are zeros, which change
//    nothing): lane l owns the terms at grid positions l, 64 + l, 128 + l,
//    ... and runs Horner's rule over them with the launch constant X^64 --
//    one step is 4 lookups in a 4 x 256 table of that constant, which the
//    workgroup builds in LDS at its start (32 basis products, then xors).
//    Every load is 64 consecutive words.
//  * The 64 lane values merge pairwise with X, X^2, ..., X^32 (6 levels, each
//    a 32-step shift/xor product by a wave-uniform constant).
//  * The segment's value is weighted with X^(r kSeg) (a product over the set
//    bits of r of the launch constants X^(kSeg 2^j)) and x^(8 L); segment 0
//    adds c_{n-1}.  A cell of one segment stores its value; a launch with
//    larger cells runs on an output the call has cleared on the stream first,
//    and every segment xors its value in (xor commutes with the byte swap of
//    a wire-order output).
//
// A workgroup is 4 waves = 4 segments; no wave waits for another after the
// table is built.  Nothing is read at or past a cell's last checksum, nor
// before its first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>

#include "crc_math.h"
#include "hdfs_crc32c.h"
#include "hdfs_crc32c_debug.h"
#include "runtime_internal.h"

namespace hdfs_crc {
namespace {

constexpr uint32_t kListCap = CRC32C_COMPOSITE_LIST_MAX_BLOCKS;
constexpr uint32_t kLanes = 64;                // lanes per segment (one wave)
constexpr uint32_t kWaves = 4;                 // segments per workgroup
constexpr uint32_t kRun = 128;                 // terms per lane at most
constexpr uint32_t kSeg = kLanes * kRun;       // terms per segment
constexpr uint32_t kSegPows = 20;              // X^(kSeg 2^j), j < 20: 2^32 checksums / kSeg segments

// The launch constants: everything that depends on bpc and the polynomial.
struct CompConst {
    uint32_t poly;
    uint32_t x64;             // X^64: the lanes' Horner constant (the LDS table)
    uint32_t xt[6];           // X^(2^j): the lane merge
    uint32_t wp[kSegPows];    // X^(kSeg 2^j): a segment's weight
    uint32_t accumulate;      // the output was cleared: xor into it
};

// Cells of one contiguous array: cell i = sums[i * cpc ...), the last ragged.
struct CompContig {
    const uint32_t *sums;
    uint32_t *out;
    uint64_t nsums;
    uint64_t ncells;
    uint32_t cpc;
    uint32_t segs;    // segments per cell
    uint32_t x_last;  // x^(8 last_len): the array's very last chunk (every other cell ends with X)
    CompConst k;
};

// Cells anywhere: the references and each cell's x^(8 last_len) ride in the
// kernel arguments, 16 bytes per cell.
struct CompList {
    const uint32_t *sums[kListCap];
    uint32_t n[kListCap];
    uint32_t xl[kListCap];
    uint32_t *out;
    uint32_t ncells;
    CompConst k;
};
static_assert(sizeof(CompList) <= 4096, "the list launch's arguments stay within 4 KiB");

// a * b mod P, reflected (bit 31 = x^0), as crc_math.cpp's mulmod: b is
// wave-uniform wherever this is called, so its 32 values are scalar work.
__device__ __forceinline__ uint32_t mulc(uint32_t a, uint32_t b, uint32_t poly) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (poly & (0u - (b & 1u)));
    }
    return p;
}

// The workgroup's table of c = X^64: tab[256 k + b] = (b << 8 k) * c.  Every
// word is written before the barrier that ends this; nothing is assumed of
// what LDS held.
__device__ __forceinline__ void build_table(uint32_t *tab, uint32_t *basis, uint32_t c, uint32_t poly) {
    const uint32_t t = threadIdx.x;
    if (t < 32) basis[t] = mulc(1u << t, c, poly);
    __syncthreads();
    for (uint32_t e = t; e < 1024; e += kLanes * kWaves) {
        const uint32_t k8 = (e >> 8) * 8, b = e & 255u;
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v ^= basis[k8 + i] & (0u - ((b >> i) & 1u));
        tab[e] = v;
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t tmul(const uint32_t *tab, uint32_t h) {
    return tab[h & 255u] ^ tab[256 + ((h >> 8) & 255u)] ^ tab[512 + ((h >> 16) & 255u)] ^ tab[768 + (h >> 24)];
}

template <bool kSwap>
__device__ __forceinline__ uint32_t value_of(uint32_t stored) {
    return kSwap ? __builtin_bswap32(stored) : stored;
}

// One wave: segment r of the cell of n checksums at src, its weighted value
// to *out.  xl = x^(8 L) of the cell's last chunk.  r and n are wave-uniform.
template <bool kSwap>
__device__ __forceinline__ void segment(const uint32_t *tab, const uint32_t *src, uint32_t n, uint32_t r, uint32_t xl,
                                        uint32_t *out, const CompConst &k) {
    const uint32_t lane = threadIdx.x & (kLanes - 1);
    if (n == 0) {  // (list form only) the empty cell: 0
        if (r == 0 && lane == 0 && !k.accumulate) *out = 0;
        return;
    }
    const int64_t m = int64_t(n) - 1;            // terms of H
    const int64_t hi = m - int64_t(r) * kSeg;    // this segment: terms [lo, hi)
    if (r > 0 && hi <= 0) return;                // (a ragged cell of fewer segments)
    const int64_t lo = hi > int64_t(kSeg) ? hi - int64_t(kSeg) : 0;
    const uint32_t rows = uint32_t((hi - lo + kLanes - 1) / kLanes);  // 0 for a cell of one checksum
    // Right-aligned: row q, lane l is term hi - 64 (rows - q) + l; only row 0
    // can reach before lo.
    uint32_t h = 0;
    if (rows) {
        const int64_t i0 = hi - int64_t(rows) * kLanes + lane;
        if (i0 >= lo) h = value_of<kSwap>(src[i0]);
        const uint32_t *p = src + (i0 + kLanes);
#pragma unroll 4
        for (uint32_t q = 1; q < rows; ++q, p += kLanes) h = tmul(tab, h) ^ value_of<kSwap>(*p);
    }
    // lanes merge: after level j the lanes with bits 0..j set hold the value
    // of their 2^(j+1) lanes (the other lanes' values are not used)
#pragma unroll
    for (int j = 0; j < 6; ++j) h = mulc(__shfl_xor(h, 1 << j), k.xt[j], k.poly) ^ h;
    uint32_t v = __builtin_amdgcn_readlane(h, kLanes - 1);
    for (uint32_t j = 0; j < kSegPows; ++j)
        if ((r >> j) & 1u) v = mulc(v, k.wp[j], k.poly);
    v = mulc(v, xl, k.poly);
    if (r == 0) v ^= value_of<kSwap>(src[m]);
    if (lane == 0) {
        const uint32_t s = value_of<kSwap>(v);  // (stored in the order the inputs are stored in)
        if (k.accumulate)
            atomicXor(out, s);
        else
            *out = s;
    }
}

template <bool kSwap>
__global__ __launch_bounds__(kLanes *kWaves) void hdfs_composite_cells_kernel(const CompContig p) {
    __shared__ uint32_t tab[1024];
    __shared__ uint32_t basis[32];
    build_table(tab, basis, p.k.x64, p.k.poly);
    const uint64_t w = uint64_t(blockIdx.x) * kWaves + threadIdx.x / kLanes;
    const uint64_t cell = p.segs == 1 ? w : w / p.segs;
    if (cell >= p.ncells) return;
    const uint32_t r = p.segs == 1 ? 0u : uint32_t(w % p.segs);
    const uint64_t first = cell * p.cpc;
    const uint32_t n = uint32_t(std::min<uint64_t>(p.cpc, p.nsums - first));
    const uint32_t xl = cell + 1 == p.ncells ? p.x_last : p.k.xt[0];
    segment<kSwap>(tab, p.sums + first, n, r, xl, p.out + cell, p.k);
}

// grid (cells, groups of kWaves segments): a workgroup past its cell's
// segments leaves at once.
template <bool kSwap>
__global__ __launch_bounds__(kLanes *kWaves) void hdfs_composite_list_kernel(const CompList p) {
    __shared__ uint32_t tab[1024];
    __shared__ uint32_t basis[32];
    const uint32_t cell = blockIdx.x;
    const uint32_t n = p.n[cell];
    const uint32_t segs = n > kSeg + 1 ? uint32_t((uint64_t(n) + kSeg - 2) / kSeg) : 1u;
    if (blockIdx.y * kWaves >= segs) return;
    build_table(tab, basis, p.k.x64, p.k.poly);
    const uint32_t r = blockIdx.y * kWaves + threadIdx.x / kLanes;
    if (r >= segs) return;
    segment<kSwap>(tab, p.sums[cell], n, r, p.xl[cell], p.out + cell, p.k);
}

inline uint32_t segments_of(uint64_t n) { return n > kSeg + 1 ? uint32_t((n - 1 + kSeg - 1) / kSeg) : 1u; }

void make_constants(uint32_t bpc, uint32_t poly, bool accumulate, CompConst *k) {
    k->poly = poly;
    k->xt[0] = xpow8(bpc, poly);
    for (int j = 1; j < 6; ++j) k->xt[j] = mulmod(k->xt[j - 1], k->xt[j - 1], poly);
    k->x64 = mulmod(k->xt[5], k->xt[5], poly);
    k->wp[0] = xpow8(uint64_t(bpc) * kSeg, poly);
    for (uint32_t j = 1; j < kSegPows; ++j) k->wp[j] = mulmod(k->wp[j - 1], k->wp[j - 1], poly);
    k->accumulate = accumulate ? 1u : 0u;
}

int check_common(const crc32c_ctx *ctx, uint32_t flags, uint32_t bpc, const uint32_t *dev_crcs) {
    if (!ctx) return fail(-EINVAL, "ctx == NULL");
    if (flags & ~(CRC32C_BIG_ENDIAN | CRC32C_TYPE_CRC32))
        return fail(-EINVAL, "a composite takes only CRC32C_BIG_ENDIAN and CRC32C_TYPE_CRC32 (flags 0x%x)", flags);
    if (bpc == 0) return fail(-EINVAL, "bpc == 0");
    if (!dev_crcs) return fail(-EINVAL, "dev_crcs == NULL");
    if (uintptr_t(dev_crcs) & 3u) return fail(-EINVAL, "dev_crcs is not 4-byte aligned");
    return 0;
}

// The list launches of (dev_sums[i], nsums[i] or same_n, last_lens[i] or
// same_last) -> dev_crcs[i]; the arguments are checked already.
int launch_list(const crc32c_ctx *ctx, const uint32_t *const *dev_sums, const uint32_t *nsums, uint32_t same_n,
                const uint32_t *last_lens, uint32_t same_last, size_t ncells, uint32_t bpc, uint32_t flags,
                uint32_t *dev_crcs, hipStream_t s) {
    const uint32_t poly = (flags & CRC32C_TYPE_CRC32) ? kPolyIeee : kPoly;
    uint32_t max_n = nsums ? 0 : same_n;
    if (nsums)
        for (size_t i = 0; i < ncells; ++i) max_n = std::max(max_n, nsums[i]);
    const bool accumulate = segments_of(max_n) > 1;
    DeviceGuard guard(ctx->device);
    if (accumulate) HIP_TRY(hipMemsetAsync(dev_crcs, 0, 4 * ncells, s));
    CompList p;
    make_constants(bpc, poly, accumulate, &p.k);
    uint32_t cached_len = 0, cached_xl = 0;
    for (size_t i = 0; i < ncells; i += kListCap) {
        const uint32_t c = uint32_t(std::min<size_t>(kListCap, ncells - i));
        uint32_t launch_max = 0;
        for (uint32_t j = 0; j < c; ++j) {
            p.sums[j] = dev_sums[i + j];
            p.n[j] = nsums ? nsums[i + j] : same_n;
            const uint32_t len = p.n[j] ? (last_lens ? last_lens[i + j] : same_last) : 0;
            if (len != cached_len) {
                cached_len = len;
                cached_xl = xpow8(len, poly);
            }
            p.xl[j] = len ? cached_xl : 0u;
            launch_max = std::max(launch_max, p.n[j]);
        }
        p.out = dev_crcs + i;
        p.ncells = c;
        const dim3 g{c, (segments_of(launch_max) + kWaves - 1) / kWaves, 1}, b{kLanes * kWaves, 1, 1};
        if (flags & CRC32C_BIG_ENDIAN)
            hipLaunchKernelGGL(hdfs_composite_list_kernel<true>, g, b, 0, s, p);
        else
            hipLaunchKernelGGL(hdfs_composite_list_kernel<false>, g, b, 0, s, p);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

// Loads this file's code object onto the current device (crc32c_ctx_create,
// beside preload_md5_kernels).
hipError_t preload_composite_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&hdfs_composite_cells_kernel<true>));
}

}  // namespace hdfs_crc

using namespace hdfs_crc;

extern "C" {

void crc32c_debug_composite_geometry(crc32c_debug_composite_geom *out) {
    if (!out) return;
    out->run = kRun;
    out->lanes = kLanes;
    out->waves_per_workgroup = kWaves;
    out->split_above = kSeg + 1;
}

int crc32c_composite_cells(crc32c_ctx *ctx, const uint32_t *dev_sums, uint64_t nsums, uint32_t crc_per_cell,
                           uint32_t bpc, uint32_t last_len, uint32_t flags, uint32_t *dev_crcs, void *stream) {
    if (int rc = check_common(ctx, flags, bpc, dev_crcs)) return rc;
    if (nsums == 0) return 0;
    if (crc_per_cell == 0) return fail(-EINVAL, "crc_per_cell == 0");
    if (last_len == 0 || last_len > bpc) return fail(-EINVAL, "last_len %u is not in 1 .. bpc (%u)", last_len, bpc);
    if (!dev_sums) return fail(-EINVAL, "dev_sums == NULL");
    if (uintptr_t(dev_sums) & 3u) return fail(-EINVAL, "dev_sums is not 4-byte aligned");
    const uint32_t poly = (flags & CRC32C_TYPE_CRC32) ? kPolyIeee : kPoly;
    CompContig p;
    p.sums = dev_sums;
    p.out = dev_crcs;
    p.nsums = nsums;
    p.ncells = crc32c_md5_nblocks(nsums, crc_per_cell);
    p.cpc = crc_per_cell;
    p.segs = segments_of(std::min<uint64_t>(crc_per_cell, nsums));
    p.x_last = xpow8(last_len, poly);
    make_constants(bpc, poly, p.segs > 1, &p.k);
    const uint64_t grid = (p.ncells * p.segs + kWaves - 1) / kWaves;
    if (p.ncells > (1ull << 40) || grid > 0x7fffffffull)
        return fail(-EINVAL, "%llu cells are more than one launch holds", (unsigned long long)p.ncells);
    DeviceGuard guard(ctx->device);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.segs > 1) HIP_TRY(hipMemsetAsync(dev_crcs, 0, 4 * p.ncells, s));
    const dim3 g{uint32_t(grid), 1, 1}, b{kLanes * kWaves, 1, 1};
    if (flags & CRC32C_BIG_ENDIAN)
        hipLaunchKernelGGL(hdfs_composite_cells_kernel<true>, g, b, 0, s, p);
    else
        hipLaunchKernelGGL(hdfs_composite_cells_kernel<false>, g, b, 0, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

int crc32c_composite_block_list(crc32c_ctx *ctx, const uint32_t *const *dev_sums, const uint32_t *nsums,
                                const uint32_t *last_lens, size_t nblocks, uint32_t bpc, uint32_t flags,
                                uint32_t *dev_crcs, void *stream) {
    if (int rc = check_common(ctx, flags, bpc, dev_crcs)) return rc;
    if (nblocks == 0) return 0;
    if (!dev_sums || !nsums || !last_lens) return fail(-EINVAL, "dev_sums/nsums/last_lens == NULL");
    for (size_t i = 0; i < nblocks; ++i) {
        if (!nsums[i]) continue;
        if (!dev_sums[i]) return fail(-EINVAL, "block %zu: %u checksums at NULL", i, nsums[i]);
        if (uintptr_t(dev_sums[i]) & 3u) return fail(-EINVAL, "block %zu: checksums not 4-byte aligned", i);
        if (last_lens[i] == 0 || last_lens[i] > bpc)
            return fail(-EINVAL, "block %zu: last_len %u is not in 1 .. bpc (%u)", i, last_lens[i], bpc);
    }
    return launch_list(ctx, dev_sums, nsums, 0, last_lens, 0, nblocks, bpc, flags, dev_crcs,
                       static_cast<hipStream_t>(stream));
}

int crc32c_plan_exec_blocks_composite(crc32c_plan *plan, const void *const *dev_payloads, uint32_t *const *dev_outs,
                                      size_t nblocks, uint32_t *dev_crcs, void *stream) {
    if (!plan) return fail(-EINVAL, "plan == NULL");
    uint32_t bpc = 0, last = 0;
    if (int rc = crc32c_plan_composite_shape(plan, &bpc, &last)) return rc;
    const uint32_t flags = plan->flags & (CRC32C_BIG_ENDIAN | CRC32C_TYPE_CRC32);
    if (int rc = check_common(plan->ctx, flags, bpc, dev_crcs)) return rc;
    if (plan->nchecksums > UINT32_MAX) return fail(-EINVAL, "a block of more than 2^32 - 1 checksums");
    if (nblocks == 0) return 0;
    if (!dev_payloads || !dev_outs) return fail(-EINVAL, "payloads/outs == NULL");
    for (size_t i = 0; i < nblocks; ++i)
        if (!dev_outs[i] || (uintptr_t(dev_outs[i]) & 3u))
            return fail(-EINVAL, "block %zu: out NULL / not 4-byte aligned", i);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    // (exec_blocks checks the rest before it launches anything)
    if (int rc = exec_blocks(plan, dev_payloads, dev_outs, nblocks, s, nullptr)) return rc;
    return launch_list(plan->ctx, dev_outs, nullptr, uint32_t(plan->nchecksums), nullptr, last, nblocks, bpc, flags,
                       dev_crcs, s);
}

}  // extern "C"
