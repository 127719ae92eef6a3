// crc32c_kernel.hip -- the production instantiations of the CDNA4 (gfx950)
// CRC32C chunk kernel (device code and design notes: crc32c_device.h).
//
// libhdfs_crc32c.so ships the slicing-by-4 kernel with non-temporal payload
// loads, 12 waves (768 threads) per workgroup and one workgroup per CU, in
// these builds, each storing checksums (crc32c_plan_exec) or comparing them
// (crc32c_plan_verify):
//   * full image (its split form: 16 columns per byte table, 88 KiB staged),
//     power-of-two tiles only: the bulk path (config 2);
//   * full image with the general-tile code (bpc outside 512 * 2^k, packet
//     tails) and the shifted loads of tiles off 16-byte alignment, in three
//     forms: both paths, general tiles only, shifted tiles only (a build
//     without the path a batch does not need has its registers and schedule
//     to the other path); the both-paths form, which padded chunks run,
//     computes a general item's next subtile facts ahead (kModeGHoist);
//   * compact image (28 KiB staged instead of 88 KiB, with the general-tile
//     code): batches of at most kSmallBatchItemsPerCu work items per CU,
//     where the table staging is most of a launch (one 4 MiB block: 5.8 ->
//     5.2 us);
//   * the same with quarter units (each tile split over 4 waves, 2 pieces
//     per lane): batches of at most kQuarterTilesPerCu tiles per CU, where
//     one wave's load -> lookups chain is the launch (one 4 MiB block,
//     graph-replayed: 4.36 -> 3.71 us); up to kEarlyTilesPerCu tiles per
//     CU with the first unit's loads issued before the table staging (their
//     latencies overlap: one 4 MiB block 3.71-3.74 -> 3.57 us; at 3 tiles
//     per CU the staging queues behind them, 4.16-4.22 -> 4.41-4.46, round 6);
//     a batch with no general tiles and no tile off 16-byte alignment (a
//     whole aligned block) runs that form without the general-tile code and
//     with 8 waves per workgroup, one per unit (one 4 MiB block 3.57 ->
//     3.42 us without the code, -> 3.35 us with 8 waves, round 6);
//   * the same with half units (each tile over 2 waves): batches of more
//     than kQuarterTilesPerCu and at most kHalvesTilesPerCu tiles per CU
//     (2-3 blocks: 896 tiles 5.23-5.27 -> 4.69-4.73 us, 1024 tiles
//     5.29-5.35 -> 4.76-4.82, 1536 tiles 6.09-6.16 -> 5.73-5.79, round 6);
//   * full image with the general-tile code and half tiles (bpc <= 256,
//     513..768 and 1025..1280), with and without the shifted loads, for any batch holding
//     half tiles (compiled into the builds above, their code cost those
//     3-8 %).
// A/B and diagnostic variants are built only into libhdfs_crc32c_debug.so
// (debug/crc32c_variants.hip).
#include <hip/hip_ext.h>

#include "crc32c_device.h"

namespace hdfs_crc {

// Launches the instantiation select_plan_build (plan_select.h, with the
// thresholds and their measurements) names for p, on the grid it gives.
hipError_t launch_plan_kernel(const KParams &p, uint32_t num_cu, hipStream_t stream, hipEvent_t stop,
                              uint32_t *grid) {
    using namespace hdfs_crc_dev;
    constexpr int kProd = kModeS4 | kModeNt;
    constexpr int kGen = kModeGeneral;
    constexpr int kSmall = kModeS4C | kModeGeneral | kModeNoPadT;
    constexpr int kQuarter = kSmall | kModeQuarter;
    const PlanBuild sel = select_plan_build(p.ntiles, p.ngen, p.nseg, p.nconst, p.general, p.expect != nullptr, num_cu);
    const dim3 g{sel.grid, 1, 1}, b{sel.threads, 1, 1};
    if (grid) *grid = g.x;
    if (p.expect && (!p.result || !p.sched)) return hipErrorInvalidValue;
    // Every production build, exec and verify twin: the kernels of the product library.
#define BUILD(T, W, M)                                                                                          \
    case (M):                                                                                                   \
        if (sel.threads != T || sel.waves_per_simd != W) return hipErrorInvalidValue;                           \
        if (stop)                                                                                               \
            hipExtLaunchKernelGGL((hdfs_crc32c_plan_kernel<T, W, (M)>), g, b, 0, stream, nullptr, stop, 0u, p); \
        else                                                                                                    \
            hipLaunchKernelGGL((hdfs_crc32c_plan_kernel<T, W, (M)>), g, b, 0, stream, p);                       \
        break;
#define BUILD2(T, W, M) BUILD(T, W, M) BUILD(T, W, (M) | kModeVerify)
    switch (sel.mode) {
        BUILD2(768, 3, kProd | kGen | kModeGHoist | kModeHalfT)
        BUILD2(768, 3, kProd | kGen | kModeNoShift | kModeHalfT)
        BUILD2(512, 2, kProd | kModeS4C | kModeQuarter | kModeEarly)
        BUILD2(768, 3, kProd | kQuarter | kModeEarly)
        BUILD2(768, 3, kProd | kQuarter)
        BUILD2(768, 3, kProd | kQuarter | kModeHalves)
        BUILD2(768, 3, kProd | kSmall)
        BUILD2(768, 3, kProd | kGen | kModeNoShift)
        BUILD2(768, 3, kProd | kGen | kModeNoGItems)
        BUILD2(768, 3, kProd | kGen | kModeGHoist)
        BUILD2(768, 3, kProd)
    default: return hipErrorInvalidValue;  // (a build the selector names and this library does not hold)
    }
#undef BUILD2
#undef BUILD
    return hipGetLastError();
}

// Loads this file's code object (every build above) onto the current
// device: HIP loads it at its first use, which would otherwise land in the
// process's first checksum call (1.2-2.2 ms against 16 us,
// tools/first_call_probe.py).  crc32c_ctx_create calls it.
hipError_t preload_plan_kernels() {
    using namespace hdfs_crc_dev;
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&hdfs_crc32c_plan_kernel<768, 3, kModeS4 | kModeNt>));
}

}  // namespace hdfs_crc
