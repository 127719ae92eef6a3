// crc32c_verdicts.hip -- per-cell verdicts from a mismatch bitmap on the GPU
// (include/hdfs_crc32c.h section 6d, and the last launch of
// crc32c_plan_verify_blocks, section 3c): the bitmap a verify launch left in
// device memory, cut into cells of crc_per_cell bits, gives each cell's
// mismatch count and its lowest and highest mismatching index.
//
// No atomics and no clearing pass: every verdict is written whole by exactly
// one lane, so nothing needs initialising and a graph replay is idempotent.
// Two forms, chosen by the cell size (wave64, gfx950):
//  * LANE form, cells of at most kLaneMaxCell bits: one lane per cell; the
//    lane reads its cell's words (at most kLaneMaxCell / 32 + 1) itself.
//  * WAVE form, larger cells: one wave per cell; lane l reads words w0 + l,
//    w0 + 64 + l, ... of the cell (64 consecutive words per load
//    instruction), masks the cell's first and last word (a neighbour's bits
//    in a shared word, the bits at and past nsums), takes popcount and first
//    / last set bit per word, and the 64 lanes merge with a sum / min / max
//    butterfly.  A cell is never split over waves: one very large cell is
//    its wave's loop (262 144 bits: 128 loads per lane).
// The grid is capped (kGridCap workgroups of kWaves waves) and strides over
// the cells.  Nothing is read past word ceil(nsums / 32) - 1.
//
// The internal form (crc32c_plan_verify_blocks) also takes the verify
// launches' results: cell i ORs bit 31 (CRC32C_VERIFY_OVERLAP) of
// group_results[2 (i / cells_per_group)] into its mismatches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>

#include "hdfs_crc32c.h"
#include "hdfs_crc32c_debug.h"
#include "runtime_internal.h"
#include "verdict_cell.h"

namespace hdfs_crc {
namespace {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kWaves = 4;            // waves per workgroup
constexpr uint32_t kLaneMaxCell = 128;    // bits: the largest cell one lane reads (5 words at most)
constexpr uint32_t kGridCap = 1024;       // workgroups: 256 CUs x 4

struct VerdictParams {
    const uint32_t *bits;
    crc32c_block_verdict *out;
    uint64_t nsums;
    uint64_t ncells;
    uint32_t cpc;
    uint32_t cells_per_group;        // (group_results != null)
    const uint32_t *group_results;   // null: no overlap bits
};

__device__ __forceinline__ void store_verdict(const VerdictParams &p, uint64_t cell, const CellAcc &a) {
    uint32_t overlap = 0;
    if (p.group_results) overlap = p.group_results[2 * (cell / p.cells_per_group)] & CRC32C_VERIFY_OVERLAP;
    p.out[cell] = cell_verdict(a, overlap);
}

__global__ __launch_bounds__(kLanes *kWaves) void hdfs_verdicts_lane_kernel(const VerdictParams p) {
    const uint64_t stride = uint64_t(gridDim.x) * (kLanes * kWaves);
    for (uint64_t cell = uint64_t(blockIdx.x) * (kLanes * kWaves) + threadIdx.x; cell < p.ncells; cell += stride) {
        const uint64_t b0 = cell * p.cpc, b1 = std::min<uint64_t>(b0 + p.cpc, p.nsums);
        CellAcc a;
        for (uint64_t w = b0 >> 5; w <= (b1 - 1) >> 5; ++w)
            cell_add_word(a, p.bits[w] & cell_word_mask(w, b0, b1), w, b0);
        store_verdict(p, cell, a);
    }
}

__global__ __launch_bounds__(kLanes *kWaves) void hdfs_verdicts_wave_kernel(const VerdictParams p) {
    const uint32_t lane = threadIdx.x & (kLanes - 1);
    const uint64_t stride = uint64_t(gridDim.x) * kWaves;
    for (uint64_t cell = uint64_t(blockIdx.x) * kWaves + threadIdx.x / kLanes; cell < p.ncells; cell += stride) {
        const uint64_t b0 = cell * p.cpc, b1 = std::min<uint64_t>(b0 + p.cpc, p.nsums);  // (wave-uniform)
        const uint64_t w1 = (b1 - 1) >> 5;
        CellAcc a;
        for (uint64_t w = (b0 >> 5) + lane; w <= w1; w += kLanes)
            cell_add_word(a, p.bits[w] & cell_word_mask(w, b0, b1), w, b0);
        // the 64 lanes merge: after level j every lane holds the value of its 2^(j+1) lanes
#pragma unroll
        for (int j = 0; j < 6; ++j)
            cell_merge(a, __shfl_xor(a.count, 1 << j), __shfl_xor(a.first, 1 << j), __shfl_xor(a.last, 1 << j));
        if (lane == 0) store_verdict(p, cell, a);
    }
}

}  // namespace

// The verdict launch over a checked bitmap (nsums > 0, crc_per_cell > 0,
// pointers 4-byte aligned); group_results: the internal form.
int launch_verdicts(const crc32c_ctx *ctx, const uint32_t *dev_bad_bits, uint64_t nsums, uint32_t crc_per_cell,
                    crc32c_block_verdict *dev_verdicts, const uint32_t *group_results, uint32_t cells_per_group,
                    hipStream_t s) {
    VerdictParams p;
    p.bits = dev_bad_bits;
    p.out = dev_verdicts;
    p.nsums = nsums;
    p.ncells = crc32c_md5_nblocks(nsums, crc_per_cell);
    p.cpc = crc_per_cell;
    p.cells_per_group = group_results ? cells_per_group : 1u;
    p.group_results = group_results;
    const bool lane_form = crc_per_cell <= kLaneMaxCell;
    const uint64_t per_wg = lane_form ? kLanes * kWaves : kWaves;
    const dim3 g{uint32_t(std::min<uint64_t>((p.ncells + per_wg - 1) / per_wg, kGridCap)), 1, 1}, b{kLanes * kWaves, 1, 1};
    DeviceGuard guard(ctx->device);
    if (lane_form)
        hipLaunchKernelGGL(hdfs_verdicts_lane_kernel, g, b, 0, s, p);
    else
        hipLaunchKernelGGL(hdfs_verdicts_wave_kernel, g, b, 0, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Loads this file's code object onto the current device (crc32c_ctx_create,
// beside preload_composite_kernels).
hipError_t preload_verdict_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&hdfs_verdicts_wave_kernel));
}

}  // namespace hdfs_crc

using namespace hdfs_crc;

extern "C" {

void crc32c_debug_verdict_geometry(crc32c_debug_verdict_geom *out) {
    if (!out) return;
    out->lane_max_cell = kLaneMaxCell;
    out->lanes = kLanes;
    out->waves_per_workgroup = kWaves;
    out->grid_cap = kGridCap;
}

int crc32c_bitmap_verdicts(crc32c_ctx *ctx, const uint32_t *dev_bad_bits, uint64_t nsums, uint32_t crc_per_cell,
                           crc32c_block_verdict *dev_verdicts, void *stream) {
    if (!ctx) return fail(-EINVAL, "ctx == NULL");
    if (nsums == 0) return 0;
    if (crc_per_cell == 0) return fail(-EINVAL, "crc_per_cell == 0");
    if (!dev_bad_bits || !dev_verdicts) return fail(-EINVAL, "dev_bad_bits/dev_verdicts == NULL");
    if ((uintptr_t(dev_bad_bits) | uintptr_t(dev_verdicts)) & 3u)
        return fail(-EINVAL, "dev_bad_bits/dev_verdicts not 4-byte aligned");
    return launch_verdicts(ctx, dev_bad_bits, nsums, crc_per_cell, dev_verdicts, nullptr, 0,
                           static_cast<hipStream_t>(stream));
}

}  // extern "C"
