/* file_composite_crc.c -- a file's composite CRC (Hadoop's COMPOSITE_CRC block
 * checksums and its COMPOSITE-CRC32C file checksum) computed from C through
 * libhdfs_crc32c.so with the file's blocks in device memory (INTEGRATION.md,
 * "Composite CRCs"):
 *   1. the blocks are filled in device memory (one allocation each);
 *   2. one plan of a block's packets (crc32c_packetize, 64 KiB packets), and
 *      a second one when the last block has another length;
 *      crc32c_plan_composite_shape tells that each combines;
 *   3. crc32c_plan_exec_blocks_composite per block shape: every block's
 *      checksums and then the CRC of the block's bytes combined from them,
 *      on one stream, nothing copied back in between;
 *   4. the n block CRCs are copied back;
 *   5. crc32c_file_composite over them and the block lengths is the file
 *      checksum's value;
 *   6. it is checked against the drop-in scalar crc32c() over the whole
 *      file, and every block CRC against crc32c() over that block;
 *   7. "ok: <file CRC as 8 hex digits = its 4 big-endian wire bytes>".
 *
 * Fill pattern: block i holds the xorshift64 (13, 7, 17) stream seeded with
 * 0x9E3779B97F4A7C15 + i, each state after the step emitted as 8
 * little-endian bytes (the last state cut to the block's length).
 *
 *   file_composite_crc nblocks block_len last_block_len bpc
 * blocks 0 .. nblocks - 2 hold block_len bytes, the last one last_block_len.
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
 * packet order.  Returns the packet count; *nsums = the block's checksums. */
static size_t block_packets(uint64_t len, uint32_t bpc, crc32c_packet **out, uint64_t *nsums) {
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
    *nsums = idx;
    return (size_t)np;
}

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s nblocks block_len last_block_len bpc\n", argv[0]);
        return 2;
    }
    const size_t nblocks = (size_t)strtoull(argv[1], NULL, 0);
    const uint64_t block_len = strtoull(argv[2], NULL, 0), last_len = strtoull(argv[3], NULL, 0);
    const uint32_t bpc = (uint32_t)strtoul(argv[4], NULL, 0);
    if (!nblocks || !bpc || !block_len || !last_len) {
        fprintf(stderr, "nblocks, the lengths and bpc must be positive\n");
        return 2;
    }
    const size_t nwhole = block_len == last_len ? nblocks : nblocks - 1; /* blocks of the first plan */
    const uint64_t maxlen = block_len > last_len ? block_len : last_len;

    /* 1. the blocks, on the host (one buffer: the file) and in device memory */
    const uint64_t file_len = block_len * (nblocks - 1) + last_len;
    uint8_t *file = malloc(file_len + 1);
    uint64_t *lens = calloc(nblocks, sizeof *lens);
    const void **d_blocks = calloc(nblocks, sizeof *d_blocks);
    for (size_t i = 0; i < nblocks; ++i) {
        lens[i] = i + 1 < nblocks ? block_len : last_len;
        uint8_t *h = file + block_len * i;
        fill_block(h, lens[i], 0x9E3779B97F4A7C15ull + i);
        void *d = NULL;
        HIP_OK(hipMalloc(&d, lens[i] + 16));
        HIP_OK(hipMemcpy(d, h, lens[i], hipMemcpyHostToDevice));
        d_blocks[i] = d;
    }

    crc32c_ctx *ctx = NULL;
    int rc = crc32c_ctx_create(0, &ctx);
    CHECK(rc == 0, "ctx_create: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;

    /* 2. one plan per block shape */
    crc32c_packet *pk[2] = {NULL, NULL};
    size_t npk[2] = {0, 0};
    uint64_t nsums[2] = {0, 0};
    crc32c_plan *plan[2] = {NULL, NULL};
    npk[0] = block_packets(nwhole ? block_len : last_len, bpc, &pk[0], &nsums[0]);
    npk[1] = block_packets(last_len, bpc, &pk[1], &nsums[1]);
    for (int s = 0; s < 2; ++s) {
        rc = crc32c_plan_create(ctx, pk[s], npk[s], 0, &plan[s]);
        CHECK(rc == 0, "plan_create: %d (%s)", rc, crc32c_last_error());
        if (rc) return 1;
        uint32_t sb = 0, sl = 0;
        const uint64_t len = s == 0 && nwhole ? block_len : last_len;
        rc = crc32c_plan_composite_shape(plan[s], &sb, &sl);
        CHECK(rc == 0, "plan_composite_shape: %d (%s)", rc, crc32c_last_error());
        CHECK(sb == bpc && sl == (len % bpc ? len % bpc : bpc), "shape (%u, %u) of a block of %" PRIu64 " bytes", sb,
              sl, len);
    }

    /* per-block checksum arrays and the block CRCs, in device memory */
    const uint64_t maxsums = crc32c_nchunks(maxlen, bpc) + maxlen / 65536 + 2;
    uint32_t **d_sums = calloc(nblocks, sizeof *d_sums);
    for (size_t i = 0; i < nblocks; ++i) HIP_OK(hipMalloc((void **)&d_sums[i], maxsums * 4));
    uint32_t *d_crcs = NULL;
    HIP_OK(hipMalloc((void **)&d_crcs, 4 * nblocks));
    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));

    /* 3. checksums, then the block CRCs combined from them, on one stream */
    rc = crc32c_plan_exec_blocks_composite(plan[0], d_blocks, d_sums, nwhole, d_crcs, stream);
    CHECK(rc == 0, "plan_exec_blocks_composite: %d (%s)", rc, crc32c_last_error());
    if (nwhole < nblocks) {
        rc = crc32c_plan_exec_blocks_composite(plan[1], d_blocks + nwhole, d_sums + nwhole, 1, d_crcs + nwhole, stream);
        CHECK(rc == 0, "plan_exec_blocks_composite (last block): %d (%s)", rc, crc32c_last_error());
    }

    /* 4. the block CRCs back; 5. the file checksum */
    uint32_t *crcs = malloc(4 * nblocks);
    HIP_OK(hipMemcpyAsync(crcs, d_crcs, 4 * nblocks, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    uint32_t file_crc = 0;
    rc = crc32c_file_composite(crcs, lens, nblocks, 0, &file_crc);
    CHECK(rc == 0, "file_composite: %d (%s)", rc, crc32c_last_error());

    /* 6. against the scalar CRC of the bytes */
    for (size_t i = 0; i < nblocks; ++i) {
        const uint32_t want = crc32c(0, file + block_len * i, lens[i]);
        CHECK(crcs[i] == want, "block %zu: composite %08x, crc32c() over its bytes %08x", i, crcs[i], want);
    }
    const uint32_t want = crc32c(0, file, file_len);
    CHECK(file_crc == want, "file: composite %08x, crc32c() over its bytes %08x", file_crc, want);

    /* 7. */
    printf("%s: %08x\n", fails ? "FAILED" : "ok", file_crc);

    for (int s = 0; s < 2; ++s) {
        crc32c_plan_destroy(plan[s]);
        free(pk[s]);
    }
    HIP_OK(hipStreamDestroy(stream));
    crc32c_ctx_destroy(ctx);
    for (size_t i = 0; i < nblocks; ++i) {
        HIP_OK(hipFree((void *)d_blocks[i]));
        HIP_OK(hipFree(d_sums[i]));
    }
    HIP_OK(hipFree(d_crcs));
    free(crcs);
    free(d_sums);
    free(d_blocks);
    free(lens);
    free(file);
    return fails ? 1 : 0;
}
