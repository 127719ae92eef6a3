// plan_select.h -- which production build of the CRC32C kernel a launch runs.
//
// Plain host C++ (no HIP): the kernel's template mode bits, the KParams::general
// bits, and select_plan_build, the one place that turns a launch's item counts
// into a kernel instantiation and a grid.  launch_plan_kernel
// (crc32c_kernel.hip) launches exactly what it names; the CPU test-suite
// checks it at every threshold through crc32c_debug_select_build.
#pragma once
#include <stdint.h>

namespace hdfs_crc_dev {

// Kernel modes (template bits).  Production = kModeS4 | kModeNt (+ kModeVerify).
constexpr int kModeNt = 1;          // payload loads non-temporal (streamed once)
constexpr int kModeS4 = 2;          // slicing-by-4 chains + per-column finishing operator (S4 image)
constexpr int kModeStamps = 4;      // DIAGNOSTIC: per-wave timestamps
constexpr int kModeMemDiag = 8;     // DIAGNOSTIC, wrong results: no lookups (memory ceiling)
constexpr int kModeCompDiag = 16;   // DIAGNOSTIC, wrong results: no payload loads (compute ceiling)
constexpr int kModeNoStage = 32;    // DIAGNOSTIC (wrong results unless the LDS already holds the image): no table staging
constexpr int kModeVerify = 64;     // read side: compare with p.expect[] instead of storing (crc32c_plan_verify)
constexpr int kModeS4C = 512;      // small batches: compact S4 image (T0..T3 once, 28 KiB staged)
constexpr int kModeEarly = 1024;    // the first tile's loads are issued before the table staging
constexpr int kModeHalves = 16384;  // with kModeQuarter, 2 units of 8 blocks per tile instead of 4 (3-6 tiles per CU)
constexpr int kModeQuarter = 4096;  // small batches: power-of-two tiles of chunks <= 2 KiB run as 4 work
                                    // units of 4 blocks each (4x the waves, 1/4 of each wave's latency chain)
constexpr int kModeXcdMap = 2048;   // A/B: workgroup ranges remapped so that each XCD's workgroups hold one
                                    // contiguous 1/8 of the batch (instead of every eighth range)
constexpr int kModeGDiagNoGather = 128;  // DIAGNOSTIC, wrong results: general items skip the per-subtile gather
constexpr int kModeGDiagNoMask = 8192;   // DIAGNOSTIC, wrong results: general items skip the chunk-start masks
constexpr int kModeGeneral = 256;   // the batch has general tiles (a plan without them runs the kernel without
                                    // their code: the power-of-two tile loop stays as compact as round 1's)
// (with kModeGeneral) the batch has no shifted tiles / no general tiles: the
// build leaves that code out, so the other path gets the registers and the
// schedule to itself
constexpr int kModeNoShift = 32768;
constexpr int kModeNoGItems = 65536;
constexpr int kModeGHoist = 131072;  // a general item's next subtile facts computed before this subtile's lookups
                                     // (the both-paths general build: padded chunks 0.5-2 % faster, round 5)
constexpr int kModeGGroup2 = 262144;  // A/B: (with kModeNoShift) general items gathered 2 subtiles at a time, not 4
constexpr int kModeHalfT = 1048576;   // (with kModeGeneral) the build also runs half tiles (their own builds: the
                                      // code costs the other general builds 3-8 %, round 5)
constexpr int kModeNoPadT = 2097152;  // (general builds) no padded power-of-two tiles: the production small-batch
                                      // builds (their code there cost config 3 ~4 %, round 5)
constexpr int kModeOvl = 524288;      // A/B: the first tile's loads issued right after the table staging's, before
                                      // the barrier that waits for the staging (their latencies overlap)
constexpr int kModeImg32 = 4194304;   // A/B (debug library only): the 32-column S4 image (152 KiB staged) instead
                                      // of the split image (88 KiB) every full-image production build stages

}  // namespace hdfs_crc_dev

namespace hdfs_crc {

constexpr uint32_t kGeneralItems = 1u, kGeneralShift = 2u, kGeneralHalf = 4u, kGeneralPadded = 8u;  // KParams::general

// Work items per CU up to which the compact image wins: its T lookups are
// not conflict-free (one copy of each table instead of 32 lane columns), so
// once every CU has many tiles the full image's faster lookups pay back its
// staging (small batches; graph-replayed, 3072 tiles:
// 7.89 vs 8.24 us, 4096: 9.05 vs 9.39, 8192: full image ahead,
// profiles/r02/launch_probe_units_crossover.json).
constexpr uint64_t kSmallBatchItemsPerCu = 16;
// Tiles per CU up to which quarter units win (tools/launch_probe.py,
// profiles/r02/launch_probe_crossover.json: 512 tiles 3.71 vs 4.36 us, 768
// tiles 4.24 vs 4.72, 1024 tiles 5.56 vs 4.95).
constexpr uint64_t kQuarterTilesPerCu = 3;
// Tiles per CU up to which the quarter-unit build issues the first unit's
// loads before the table staging (tools/launch_probe.py, debug variants 82 /
// 83, profiles/r06/early/: 512 tiles 3.57 vs 3.71-3.74 us, 768 tiles
// 4.41-4.46 vs 4.16-4.22).
constexpr uint64_t kEarlyTilesPerCu = 2;
// Tiles per CU up to which half units win over whole tiles (debug variant
// 86 against production, tools/launch_probe.py, profiles/r06/halves/: 1280
// tiles 5.50-5.55 vs 5.95-5.98 us, 1536 5.73-5.79 vs 6.09-6.16, 1792
// 6.80-6.84 vs 6.56-6.58, 2048 7.02-7.13 vs 6.79-6.94).  (Round 2 measured
// halves only with the padded-tile code in the build: 2-5 %.)
constexpr uint64_t kHalvesTilesPerCu = 6;

// Work items of a launch as its grid counts them: tiles (or their units),
// gen / seg items in pairs, constant runs.
inline uint64_t launch_items(uint32_t ntiles, uint32_t ngen, uint32_t nseg, uint32_t nconst,
                             uint32_t units_per_tile = 1) {
    return uint64_t(ntiles) * units_per_tile + (uint64_t(ngen) + 1) / 2 + (uint64_t(nseg) + 1) / 2 + nconst;
}

// Grid of a launch: one workgroup per CU, or one per work item when there
// are fewer items than CUs (a small batch leaves most waves without a tile;
// they still share the table staging, which is what bounds a small launch).
inline uint32_t production_grid(uint64_t items, uint32_t num_cu) {
    return uint32_t(items < num_cu ? (items ? items : 1) : num_cu);
}

// One production instantiation hdfs_crc32c_plan_kernel<threads,
// waves_per_simd, mode> and the grid it is launched with.
struct PlanBuild {
    uint32_t threads;
    uint32_t waves_per_simd;
    int mode;
    uint32_t units_per_tile;  // 4: quarter units, 2: half units, 1: whole tiles
    uint32_t grid;
};

// The build a launch of these item counts and KParams::general bits runs on
// num_cu CUs (verify: the comparing twin).
inline PlanBuild select_plan_build(uint32_t ntiles, uint32_t ngen, uint32_t nseg, uint32_t nconst, uint32_t general,
                                   bool verify, uint32_t num_cu) {
    using namespace hdfs_crc_dev;
    constexpr int kProd = kModeS4 | kModeNt;
    constexpr int kGen = kModeGeneral;
    constexpr int kSmall = kModeS4C | kModeGeneral | kModeNoPadT;
    constexpr int kQuarter = kSmall | kModeQuarter;
    const uint64_t items = launch_items(ntiles, ngen, nseg, nconst);
    const bool half = (general & kGeneralHalf) != 0;  // (half tiles: builds of their own, full image)
    // (padded power-of-two tiles and half tiles only run in full-image
    // builds: their code in the small-batch builds cost config 3 ~4 %)
    const bool small = !half && !(general & kGeneralPadded) && items <= kSmallBatchItemsPerCu * num_cu;
    const bool quarter = small && ntiles <= kQuarterTilesPerCu * num_cu;
    const bool early = quarter && ntiles <= kEarlyTilesPerCu * num_cu;
    const bool halves = small && !quarter && ntiles <= kHalvesTilesPerCu * num_cu;
    // Half tiles run in builds of their own, any batch size (the full image):
    // with the shifted loads only where some tile is off 16-byte alignment
    // (padded general items -- a packet's tail -- do not need them there).
    const bool half_shift = half && (general & kGeneralShift) != 0;
    PlanBuild b{768, 3, kProd, quarter ? 4u : halves ? 2u : 1u, 0};
    if (half_shift)
        b.mode = kProd | kGen | kModeGHoist | kModeHalfT;
    else if (half)
        b.mode = kProd | kGen | kModeNoShift | kModeHalfT;
    else if (early && !general) {  // (the aligned one-block form: 8 waves, one per unit)
        b.threads = 512;
        b.waves_per_simd = 2;
        b.mode = kProd | kModeS4C | kModeQuarter | kModeEarly;
    } else if (early)
        b.mode = kProd | kQuarter | kModeEarly;
    else if (quarter)
        b.mode = kProd | kQuarter;
    else if (halves)
        b.mode = kProd | kQuarter | kModeHalves;
    else if (small)
        b.mode = kProd | kSmall;
    else if (general == kGeneralItems)
        b.mode = kProd | kGen | kModeNoShift;
    else if (general == kGeneralShift)
        b.mode = kProd | kGen | kModeNoGItems;
    else if (general)
        b.mode = kProd | kGen | kModeGHoist;
    if (verify) b.mode |= kModeVerify;
    b.grid = production_grid(launch_items(ntiles, ngen, nseg, nconst, b.units_per_tile), num_cu);
    return b;
}

}  // namespace hdfs_crc
