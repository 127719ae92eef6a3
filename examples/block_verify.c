/* block_verify.c -- many blocks verified in one call from C through
 * libhdfs_crc32c.so, with the byte ranges to fetch again (INTEGRATION.md,
 * "Reading with checksums"; hdfs_crc32c.h section 3c):
 *   1. nblocks blocks are filled in device memory (one allocation each);
 *   2. one plan of a block's packets (crc32c_packetize, 64 KiB packets);
 *      crc32c_plan_exec_blocks writes every block's checksums into ONE
 *      contiguous device array (block b's at b * n) -- the "expected" values
 *      a DataNode would have sent ahead of the data;
 *   3. two blocks are corrupted: two payload bytes of block 7 % nblocks
 *      (chunks 3 and n - 2) and one expected word of block 33 % nblocks (its
 *      last chunk);
 *   4. crc32c_plan_verify_blocks: one verify launch per 32 blocks and one
 *      verdict launch, on one stream; the verdicts are copied back;
 *   5. every verdict is checked: clean blocks read {0, ~0, ~0, 0}, the
 *      corrupted ones the chunks above; the mismatch bitmap in the work area
 *      holds exactly those bits;
 *   6. one line per bad block with its re-fetch range, then
 *      "ok: <bad blocks> of <nblocks> blocks bad".
 *
 * Fill pattern: block i holds the xorshift64 (13, 7, 17) stream seeded with
 * 0x9E3779B97F4A7C15 + i, each state after the step emitted as 8
 * little-endian bytes.
 *
 *   block_verify [nblocks [block_len [bpc]]]      (40, 262144, 512)
 * block_len must give at least 6 chunks per block.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "hdfs_crc32c.h"

static int fails = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fputc('\n', stderr);                                 \
            ++fails;                                             \
        }                                                        \
    } while (0)
#define HIP_OK(call)                                                                   \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

static void fill_block(uint8_t *p, uint64_t len, uint64_t seed) {
    uint64_t s = seed, i = 0;
    while (i < len) {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        for (int b = 0; b < 8 && i < len; ++b, ++i) p[i] = (uint8_t)(s >> (8 * b));
    }
}

/* The packets hadoop_rpc_send_packets cuts a block of `len` bytes into
 * (hadooprpc.c:827-857), offsets from the block's start, checksums packed in
 * packet order.  Returns the packet count. */
static size_t block_packets(uint64_t len, uint32_t bpc, crc32c_packet **out) {
    const uint64_t np = crc32c_packetize(len, 0, 65536, bpc, NULL, 0);
    uint64_t *lens = malloc((np + 1) * sizeof *lens);
    crc32c_packet *pk = malloc((np + 1) * sizeof *pk);
    crc32c_packetize(len, 0, 65536, bpc, lens, np);
    uint64_t pos = 0, idx = 0;
    for (uint64_t p = 0; p < np; ++p) {
        pk[p].payload_off = pos;
        pk[p].out_idx = idx;
        pk[p].len = (uint32_t)lens[p];
        pk[p].bpc = bpc;
        pos += lens[p];
        idx += crc32c_nchunks(lens[p], bpc);
    }
    free(lens);
    *out = pk;
    return (size_t)np;
}

static int flip_device_byte(void *d) {
    uint8_t v = 0;
    HIP_OK(hipMemcpy(&v, d, 1, hipMemcpyDeviceToHost));
    v ^= 0x40;
    HIP_OK(hipMemcpy(d, &v, 1, hipMemcpyHostToDevice));
    return 0;
}

int main(int argc, char **argv) {
    const size_t nblocks = argc > 1 ? (size_t)strtoull(argv[1], NULL, 0) : 40;
    const uint64_t block_len = argc > 2 ? strtoull(argv[2], NULL, 0) : 262144;
    const uint32_t bpc = argc > 3 ? (uint32_t)strtoul(argv[3], NULL, 0) : 512;
    if (argc > 4 || !nblocks || !bpc || crc32c_nchunks(block_len, bpc) < 6) {
        fprintf(stderr, "usage: %s [nblocks [block_len [bpc]]]  (at least 6 chunks per block)\n", argv[0]);
        return 2;
    }

    /* 1. the blocks in device memory */
    uint8_t *h = malloc(block_len);
    void **d_blocks = calloc(nblocks, sizeof *d_blocks);
    for (size_t i = 0; i < nblocks; ++i) {
        fill_block(h, block_len, 0x9E3779B97F4A7C15ull + i);
        HIP_OK(hipMalloc(&d_blocks[i], block_len + 16));
        HIP_OK(hipMemcpy(d_blocks[i], h, block_len, hipMemcpyHostToDevice));
    }

    crc32c_ctx *ctx = NULL;
    int rc = crc32c_ctx_create(0, &ctx);
    CHECK(rc == 0, "ctx_create: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;

    /* 2. one plan; the expected checksums of every block, contiguous */
    crc32c_packet *pk = NULL;
    const size_t npk = block_packets(block_len, bpc, &pk);
    crc32c_plan *plan = NULL;
    rc = crc32c_plan_create(ctx, pk, npk, 0, &plan);
    CHECK(rc == 0, "plan_create: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;
    const uint64_t n = crc32c_plan_nchecksums(plan);
    uint32_t *d_expected = NULL;
    HIP_OK(hipMalloc((void **)&d_expected, 4 * n * nblocks));
    uint32_t **d_outs = calloc(nblocks, sizeof *d_outs);
    for (size_t i = 0; i < nblocks; ++i) d_outs[i] = d_expected + n * i;
    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    rc = crc32c_plan_exec_blocks(plan, (const void *const *)d_blocks, d_outs, nblocks, stream);
    CHECK(rc == 0, "plan_exec_blocks: %d (%s)", rc, crc32c_last_error());
    HIP_OK(hipStreamSynchronize(stream));

    /* 3. the corruption (chunk c of a block of one bpc covers bytes [c bpc, (c + 1) bpc)) */
    const size_t bad_a = 7 % nblocks, bad_b = 33 % nblocks;
    const uint32_t a_lo = 3, a_hi = (uint32_t)n - 2, b_at = (uint32_t)n - 1;
    if (flip_device_byte((uint8_t *)d_blocks[bad_a] + (uint64_t)a_lo * bpc + 5)) return 1;
    if (flip_device_byte((uint8_t *)d_blocks[bad_a] + (uint64_t)a_hi * bpc)) return 1;
    if (flip_device_byte((uint8_t *)(d_expected + n * bad_b + b_at) + 2)) return 1;

    /* 4. every block verified: one verdict each */
    const uint64_t work_bytes = crc32c_plan_verify_blocks_work_bytes(plan, nblocks);
    void *d_work = NULL;
    crc32c_block_verdict *d_verdicts = NULL;
    HIP_OK(hipMalloc(&d_work, work_bytes));
    HIP_OK(hipMalloc((void **)&d_verdicts, nblocks * sizeof *d_verdicts));
    rc = crc32c_plan_verify_blocks(plan, (const void *const *)d_blocks, d_expected, nblocks, d_verdicts, d_work, stream);
    CHECK(rc == 0, "plan_verify_blocks: %d (%s)", rc, crc32c_last_error());
    crc32c_block_verdict *v = malloc(nblocks * sizeof *v);
    uint32_t *work = malloc(work_bytes);
    HIP_OK(hipMemcpyAsync(v, d_verdicts, nblocks * sizeof *v, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(work, d_work, work_bytes, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));

    /* 5. the verdicts and the bitmap */
    size_t nbad = 0;
    for (size_t i = 0; i < nblocks; ++i) {
        uint32_t want_n = 0, want_lo = 0xffffffffu, want_hi = 0xffffffffu;
        if (i == bad_a) want_n = 2, want_lo = a_lo, want_hi = a_hi;
        if (i == bad_b) { /* (the same block when nblocks divides 26) */
            want_lo = want_n ? want_lo : b_at;
            want_hi = b_at;
            want_n += 1;
        }
        CHECK(v[i].mismatches == want_n && v[i].first_bad == want_lo && v[i].last_bad == want_hi && v[i].reserved == 0,
              "block %zu: verdict {%u, %u, %u, %u}, expected {%u, %u, %u, 0}", i, v[i].mismatches, v[i].first_bad,
              v[i].last_bad, v[i].reserved, want_n, want_lo, want_hi);
        uint32_t bits = 0;
        for (uint64_t k = n * i; k < n * (i + 1); ++k) bits += (work[k / 32] >> (k % 32)) & 1u;
        CHECK(bits == want_n, "block %zu: %u bits set in the bitmap, expected %u", i, bits, want_n);
        /* 6. */
        if (v[i].mismatches) {
            ++nbad;
            const uint64_t hi = ((uint64_t)v[i].last_bad + 1) * bpc;
            printf("bad block %zu: %u mismatches, re-fetch bytes [%" PRIu64 ", %" PRIu64 ")\n", i,
                   v[i].mismatches & ~CRC32C_VERIFY_OVERLAP, (uint64_t)v[i].first_bad * bpc,
                   hi < block_len ? hi : block_len);
        }
    }
    printf("%s: %zu of %zu blocks bad\n", fails ? "FAILED" : "ok", nbad, nblocks);

    crc32c_plan_destroy(plan);
    HIP_OK(hipStreamDestroy(stream));
    crc32c_ctx_destroy(ctx);
    for (size_t i = 0; i < nblocks; ++i) HIP_OK(hipFree(d_blocks[i]));
    HIP_OK(hipFree(d_expected));
    HIP_OK(hipFree(d_work));
    HIP_OK(hipFree(d_verdicts));
    free(pk);
    free(d_outs);
    free(d_blocks);
    free(v);
    free(work);
    free(h);
    return fails ? 1 : 0;
}
