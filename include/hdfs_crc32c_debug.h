/*
 * hdfs_crc32c_debug.h -- introspection and diagnostic hooks.
 *
 * Section 1 is exported by libhdfs_crc32c.so (host-side only, no launch):
 * the CPU test-suite checks the GPU path's host-side inputs with it without a
 * GPU -- the work decomposition and the LDS table image the kernel loads.
 *
 * Section 2 is exported only by libhdfs_crc32c_debug.so (built beside the
 * product library, linked against it): A/B and diagnostic kernel variants
 * and a plain HBM read probe, for tools/ and the bench's read-rate
 * reference.  The product library never launches anything but the
 * production kernel.  Not needed by a reference-side integration.
 */
#ifndef HDFS_CRC32C_DEBUG_H
#define HDFS_CRC32C_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#include "hdfs_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. libhdfs_crc32c.so ---- */

/* Work items a plan would upload: 16-byte FastTile {u64 src, u32 out,
 * u32 meta} (meta: nblocks | lg << 8, or bit 31 | nch * k | k << 8 |
 * nch << 13 | pad << 18 for a general tile) and 16-byte GenItem {u64 src,
 * u32 out, u32 len}.  Copies at most *_cap items; counts go to *ntiles /
 * *ngen. */
int crc32c_debug_plan(const crc32c_packet *pkts, size_t npkts, void *tiles, size_t tiles_cap, void *gen,
                      size_t gen_cap, uint64_t *ntiles, uint64_t *ngen);
/* The same with absolute != 0: the items of a plan whose payload offsets are
 * device addresses (CRC32C_DEVICE_ADDRESSES), before it is rebased. */
int crc32c_debug_plan_abs(const crc32c_packet *pkts, size_t npkts, int absolute, void *tiles, size_t tiles_cap,
                          void *gen, size_t gen_cap, uint64_t *ntiles, uint64_t *ngen);

/* Item counts of a crc32c_plan_create_buffers plan (CRC32C): counts[0..5] =
 * tiles, gen items, seg items, pieces, constant runs, checksums. */
int crc32c_debug_write_plan(const crc32c_buffer *buffers, uint32_t n_buffers, uint64_t bufferoffset, uint64_t len,
                            uint64_t blockoffset, uint32_t packetsize, uint32_t bpc, uint64_t counts[6]);

/* The LDS image the nibble variant stages (returns its size; fills dst when
 * cap is large enough) and the affine constants crc32c(0, zeros(512 << lg)),
 * lg = 0..4, and crc32c(0, zeros(r)), r = 0..3. */
size_t crc32c_debug_lds_image(void *dst, size_t cap, uint32_t *c_lg5, uint32_t *c_small4);

/* The slicing-by-4 kernel's LDS image for the checksum type in `flags`
 * (byte tables T0..T3 replicated over the 32 lane columns, the per-column
 * finishing operators N_q, the Z^(512 s) shifts); returns its size and
 * fills dst when cap is large enough. */
size_t crc32c_debug_lds_image_s4(void *dst, size_t cap, uint32_t flags);
/* The split form of that image, which the large-batch builds and the
 * resident kernel stage: 16 columns of each byte table, T_m[b] at b * 256 +
 * m * 64 + 4 c (c = 0..15), then the N_q and Z^(512 s) sections unchanged
 * (at 65536 and 81920). */
size_t crc32c_debug_lds_image_s4_split(void *dst, size_t cap, uint32_t flags);
/* The affine constants of the checksum type in `flags` (CRC32C_TYPE_CRC32 or not). */
void crc32c_debug_affine_constants(uint32_t flags, uint32_t *c_lg5, uint32_t *c_small4);

/* Fault injection for the block queue's error path (tests): the worker fails
 * the issue of the next `n` flushes of q as if their launch had failed
 * (-EIO, nothing launched); the waits of exactly those flushes' tickets
 * return the error. */
int crc32c_debug_blocks_fail_flushes(crc32c_blocks *q, uint32_t n);

/* Resident queues only: hold != 0 keeps the kernel from being launched
 * (submits queue up in the ring; 0 launches what is queued), and the next
 * fail_waits waits -- a submit's wait for a busy slot included -- return
 * -ETIMEDOUT at once. */
int crc32c_debug_blocks_resident_inject(crc32c_blocks *q, int hold, uint32_t fail_waits);

/* CPU time the queue's worker thread has used so far (its thread CPU clock),
 * in ns: what the queue itself costs beside the submitting threads. */
int crc32c_debug_blocks_worker_cpu_ns(crc32c_blocks *q, uint64_t *ns);

/* The device address of the pooled block holding a plan's descriptors (0:
 * none): tests see a destroyed plan's block come back from the pool. */
uint64_t crc32c_debug_plan_block(const crc32c_plan *plan);

/* Captured crc32c_plan_exec launches of the context so far (hdfs_crc32c.h
 * section 3, "Captured into a HIP graph"): out[0] = execs captured, out[1] =
 * those launched with no edge from the previous captured exec, out[2] = runs
 * of overlapping execs started (a run starts at the first exec of a capture
 * and wherever an exec has to keep its stream-order edge).  No GPU work. */
int crc32c_ctx_capture_stats(crc32c_ctx *ctx, uint64_t out[3]);
/* The same for the context of a multi-GPU handle's local device `local`
 * (its shard launches never chain: they go on the plan's own exec streams). */
int crc32c_debug_multi_capture_stats(crc32c_multi *m, int local, uint64_t out[3]);

/* The production kernel build a launch runs: the instantiation
 * hdfs_crc32c_plan_kernel<threads, waves_per_simd, mode> (mode: the kernel's
 * template bits, csrc/plan_select.h), the units each tile is split into (4
 * quarter, 2 half, 1 whole) and the workgroups launched. */
typedef struct crc32c_debug_build {
    uint32_t threads, waves_per_simd, mode, units_per_tile, grid;
} crc32c_debug_build;

/* The build the library's launch path chooses for these item counts and
 * `general` bits (1 general tiles, 2 shifted loads, 4 half tiles, 8 padded
 * power-of-two tiles) on num_cu CUs; verify != 0: the comparing twin.  Pure
 * host arithmetic, no GPU.  -EINVAL for num_cu == 0 or out == NULL. */
int crc32c_debug_select_build(uint32_t ntiles, uint32_t ngen, uint32_t nseg, uint32_t nconst, uint32_t general,
                              int verify, uint32_t num_cu, crc32c_debug_build *out);

/* What crc32c_plan_exec (verify != 0: crc32c_plan_verify) of this plan on
 * dev_payload would hand the kernel -- item counts, the `general` bits (the
 * payload pointer's own misalignment included), skip_z (1: the launch stages
 * the table image without its Z^(512 s) section) -- the CU count the launch
 * is sized for, and the build chosen from them by the same selector.
 * Launches nothing.  A device-address plan takes dev_payload = NULL. */
typedef struct crc32c_debug_launch_info {
    uint32_t ntiles, ngen, nseg, nconst, general, skip_z, num_cu, reserved;
    crc32c_debug_build build;
} crc32c_debug_launch_info;
int crc32c_debug_plan_launch_info(const crc32c_plan *plan, const void *dev_payload, int verify,
                                  crc32c_debug_launch_info *out);

/* The launches crc32c_plan_exec_blocks (verify != 0: the verify launches of
 * crc32c_plan_verify_blocks, before its verdict launch) would make over
 * these blocks, in order: the blocks first_block .. first_block + nblocks - 1
 * of each, what it would hand the kernel -- ntiles over all its blocks, the
 * `general` bits (a block off 16-byte alignment included), skip_z -- the CU
 * count it is sized for and the build chosen from them by the same selector.
 * per_block = 1: the plan has items other than tiles, so it has no
 * multi-block form and the call makes one ordinary launch per block (one
 * entry each; a verify call of such a plan is refused, here as there).  The
 * entry walks the launch path's own grouping and parameter code.  Launches
 * nothing and reads no device memory.  dev_outs only enters an exec call's
 * grouping (outputs of one launch lie within 2^32 checksums); NULL: block
 * k's checksums at index k * nchecksums of one array.  Fills at most cap
 * entries of out and returns the number of launches, or -EINVAL for what the
 * call itself refuses of plan, payloads and outputs. */
typedef struct crc32c_debug_blocks_launch {
    uint32_t first_block, nblocks, ntiles, general, skip_z, num_cu, per_block, reserved;
    crc32c_debug_build build;
} crc32c_debug_blocks_launch;
int crc32c_debug_plan_blocks_launch_info(const crc32c_plan *plan, const void *const *dev_payloads,
                                         uint32_t *const *dev_outs, size_t nblocks, int verify,
                                         crc32c_debug_blocks_launch *out, size_t cap);

/* The launch-path predicates over the work items of a packet batch
 * (absolute != 0: payload offsets are device addresses): *general_bits as a
 * plan of these packets on a 16-byte aligned payload would set them, and
 * *needs_z = 1 when some item shifts by Z^(512 s).  No GPU. */
int crc32c_debug_packets_flags(const crc32c_packet *pkts, size_t npkts, int absolute, uint32_t *general_bits,
                               int *needs_z);

/* The composite-CRC kernel's geometry (csrc/crc32c_composite.hip; host only,
 * no GPU): one wave combines a segment of up to run * lanes checksums, each
 * lane up to `run` of them; a workgroup is waves_per_workgroup waves; a cell
 * of MORE than split_above checksums (run * lanes + 1: the last checksum is
 * outside the lanes' sums) is split over several waves, past
 * waves_per_workgroup * run * lanes + 1 over several workgroups, whose values
 * are xor-ed into a cleared output.  The tests place their sizes from these. */
typedef struct crc32c_debug_composite_geom {
    uint32_t run, lanes, waves_per_workgroup, split_above;
} crc32c_debug_composite_geom;
void crc32c_debug_composite_geometry(crc32c_debug_composite_geom *out);

/* The composite shape crc32c_plan_create would record for a packet batch
 * (hdfs_crc32c.h section 6c, crc32c_plan_composite_shape): 0 with *bpc /
 * *last_len, or -EINVAL when the batch is not of the shape.  No GPU. */
int crc32c_debug_packets_composite_shape(const crc32c_packet *pkts, size_t npkts, uint32_t *bpc, uint32_t *last_len);

/* The verdict kernel's geometry (csrc/crc32c_verdicts.hip, hdfs_crc32c.h
 * section 6d; host only, no GPU): a cell of at most lane_max_cell bits is
 * read by one lane, a larger one by one wave of `lanes` lanes; a workgroup is
 * waves_per_workgroup waves; a launch has at most grid_cap workgroups and
 * strides over the cells beyond them (past grid_cap * waves_per_workgroup *
 * lanes cells in the lane form, grid_cap * waves_per_workgroup in the wave
 * form).  The tests place their sizes from these. */
typedef struct crc32c_debug_verdict_geom {
    uint32_t lane_max_cell, lanes, waves_per_workgroup, grid_cap;
} crc32c_debug_verdict_geom;
void crc32c_debug_verdict_geometry(crc32c_debug_verdict_geom *out);

/* The AES/CTR kernel's geometry (csrc/aes_ctr.hip, hdfs_crc32c.h section 7;
 * host only, no GPU).  A segment is cut at the 16-byte boundaries of its
 * DESTINATION: a lane takes lane_bytes of consecutive windows, a wave
 * wave_bytes, a workgroup workgroup_bytes per pass over its grid-stride loop;
 * a segment whose first byte is off a boundary spills into one more unit than
 * its length alone fills.  list_max_segments = HDFS_AES_LIST_MAX_SEGMENTS,
 * the segments of one list launch.  These are the units of a launch that
 * fills the device: a launch of at most lanes_per_cu * CUs windows (16 bytes
 * each) gives a lane one window, one of at most twice that two, and the
 * units shrink to a quarter / a half.  The tests place their sizes from
 * these. */
typedef struct crc32c_debug_aes_geom {
    uint32_t lane_bytes, wave_bytes, workgroup_bytes, list_max_segments, lanes_per_cu;
} crc32c_debug_aes_geom;
void crc32c_debug_aes_geometry(crc32c_debug_aes_geom *out);

/* How the AES/CTR entry points would size one launch on num_cu CUs (host
 * only, no GPU; the entry points size their launches with the same
 * functions): the 16-byte windows of the launch, its wave units, the windows a
 * lane takes (1, 2 or lane_bytes / 16) and the workgroups launched.  The
 * strided call is hdfs_aes_ctr_xor_strided_dev's from dst, seg_len, nsegs and
 * dst_stride (nothing else enters the sizing; a call with nothing to do
 * reports zeros); the list call is ONE launch of hdfs_aes_ctr_xor_list_dev,
 * nsegs <= HDFS_AES_LIST_MAX_SEGMENTS (only dst and len of a segment are
 * looked at).  -EINVAL for num_cu == 0, out == NULL, more list segments than
 * one launch holds, or a strided call of more wave units than 2^64.  The GPU
 * tests assert with these that a launch took the path they name. */
typedef struct crc32c_debug_aes_launch {
    uint64_t windows, wave_units;
    uint32_t windows_per_lane, grid;
} crc32c_debug_aes_launch;
int crc32c_debug_aes_strided_launch_info(uint32_t num_cu, const void *dst, uint64_t seg_len, uint64_t nsegs,
                                         uint64_t dst_stride, crc32c_debug_aes_launch *out);
int crc32c_debug_aes_list_launch_info(uint32_t num_cu, const hdfs_aes_segment *segs, size_t nsegs,
                                      crc32c_debug_aes_launch *out);

/* The erasure-coding kernel's geometry (csrc/ec_rs.hip, hdfs_crc32c.h section
 * 8; host only, no GPU).  A unit is cut at the 16-byte boundaries of OUTPUT 0:
 * a lane takes one window of lane_bytes, a wave wave_bytes (a wave unit), a
 * workgroup workgroup_bytes per pass over its grid-stride loop; a unit whose
 * output 0 is off a boundary spills into one more window than its length
 * alone fills.  The nibble tables are held table_copies times in LDS,
 * lds_bytes_per_input bytes per input of the matrix, so a CU holds
 * min(max_workgroups_per_cu, lds_bytes_per_cu / (lds_bytes_per_input * n_in))
 * workgroups, and a launch has at most that many times the CUs, of
 * waves_per_workgroup waves each: up to that many wave units every workgroup
 * runs one wave, up to waves_per_workgroup times that many no wave loops.
 * The tests place their sizes from these. */
typedef struct crc32c_debug_ec_geom {
    uint32_t lane_bytes, wave_bytes, workgroup_bytes, waves_per_workgroup, table_copies, lds_bytes_per_input,
        lds_bytes_per_cu, max_workgroups_per_cu;
} crc32c_debug_ec_geom;
void crc32c_debug_ec_geometry(crc32c_debug_ec_geom *out);

/* ---- 2. libhdfs_crc32c_debug.so only ---- */

/* Launch of a plan with an explicit kernel variant (0 = production; see
 * debug/crc32c_variants.hip): 5, 6 and 36 write per-wave timestamps, 4 x
 * u64 per wave (s_memrealtime at start, after table staging, at exit;
 * XCC_ID << 32 | HW_ID) into dev_stamps, which must then hold 4 * (waves
 * launched) entries; 3, 4, 6 and 7 compute WRONG checksums on purpose
 * (memory-only / compute-only ceilings).  -EINVAL for a variant not built. */
int crc32c_debug_plan_exec_variant(crc32c_plan *plan, const void *dev_payload, uint32_t *dev_out,
                                   uint64_t *dev_stamps, int variant, void *stream);
/* Name of a built variant (NULL if none); *exact = 1 when it computes the
 * right checksums. */
const char *crc32c_debug_variant_name(int variant, int *exact);

/* Plain streaming read of `bytes` device bytes; writes one dword per thread
 * to dev_out (at most 2^20 dwords).  Shapes 0-7: grid x 256 threads,
 * grid-stride, 16 B per lane, 4 / 8 / 4 nt / 16 / 2 nt / 8 nt / 16 nt / 1 nt
 * loads in flight per lane; shapes 8-15: tile reads like the CRC kernel's
 * (1024 or 512 threads, 8 or 4 KiB per wave, per-workgroup ranges or
 * grid-stride tiles), see debug/stream_probe.hip.  Prices the HBM read
 * roofline this device actually delivers (tools/probe_sweep.py). */
int crc32c_debug_stream_probe(const void *dev_src, uint64_t bytes, uint32_t *dev_out, uint32_t grid, int shape,
                              void *stream);

/* A/B experiment: a RESIDENT kernel for concurrent block writes (see
 * debug/resident.hip).  The kernel stays on the GPU (all CUs, tables staged
 * once) and takes blocks from a ring the submitting threads fill; it exits on
 * destroy, after idle_us (0: 2000) with nothing queued, or when stuck, and
 * submit / wait relaunch it on demand.  The plan must be aligned
 * power-of-two tiles only (one block's shape); payloads 16-byte aligned.
 * While it runs it holds every CU's LDS: other kernels wait. */
typedef struct crc32c_resident crc32c_resident;
int crc32c_debug_resident_create(crc32c_plan *plan, uint32_t idle_us, crc32c_resident **out);
int crc32c_debug_resident_submit(crc32c_resident *r, const void *dev_payload, uint32_t *dev_out, uint64_t *ticket);
int crc32c_debug_resident_wait(crc32c_resident *r, uint64_t ticket);
int crc32c_debug_resident_stats(const crc32c_resident *r, uint64_t *launches);
/* Trace of a resident runner created with HDFS_CRC32C_RESIDENT_STAMPS=1:
 * ends the running launch (a later submit relaunches), then copies 4 x u64
 * s_memrealtime stamps (100 MHz) per ticket t at [4 (t % 4096)]: forwarded,
 * seen by workgroup 0's worker, that worker's tiles stored, completed by the
 * collector; and the sum / count of the forwarder's host-slot poll round
 * trips (ticks). -EINVAL without the trace. */
int crc32c_debug_resident_trace(crc32c_resident *r, uint64_t *stamps, uint64_t *rtt_ticks, uint64_t *rtt_polls);
int crc32c_debug_resident_destroy(crc32c_resident *r);

/* Cold-LDS tests (debug/lds_poison.hip).  Poison: 4 x CUs workgroups of 256
 * threads, each holding a CU's whole LDS (163 840 bytes: one fits per CU),
 * write word i of it with (seed ^ i * 0x9E3779B9) | 1 -- a kernel launched
 * next on the stream that stages too little of its table image reads this
 * instead of the image an earlier launch left.  Peek: the same grid counts,
 * per workgroup, the words still holding that pattern into dev_counts (one
 * u32 per workgroup, zeroed by the call on the stream).  Both return the
 * number of workgroups (peek with dev_counts == NULL: that only, no launch)
 * or -errno; they run on the current device. */
int crc32c_debug_lds_poison(uint32_t seed, void *stream);
int crc32c_debug_lds_peek(uint32_t seed, uint32_t *dev_counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif
