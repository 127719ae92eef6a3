/* file_checksum.c -- a file's MD5-of-MD5-of-CRC checksum (Hadoop's
 * MD5MD5CRC32C file checksum; per block the OpBlockChecksumResponseProto.md5
 * of datatransfer.proto:262-267) computed from C through libhdfs_crc32c.so
 * with the file's blocks in device memory ("Block
 * MD5-of-CRCs"):
 *   1. the blocks are filled in device memory (one allocation each);
 *   2. one plan of a block's packets (crc32c_packetize, 64 KiB packets) with
 *      CRC32C_BIG_ENDIAN, and a second one when the last block has another
 *      length;
 *   3. crc32c_plan_exec_blocks_md5: every block's checksums and then their
 *      MD5, on one stream, nothing copied back in between;
 *   4. the 16 n digest bytes are copied back;
 *   5. crc32c_file_md5 over them is the file checksum's digest;
 *   6. every block digest is checked against crc32c_block_md5 (host) over
 *      checksums recomputed with the drop-in crc32c() per chunk;
 *   7. "ok: <hex file digest>".
 *
 * Fill pattern: block i holds the xorshift64 (13, 7, 17) stream seeded with
 * 0x9E3779B97F4A7C15 + i, each state after the step emitted as 8
 * little-endian bytes (the last state cut to the block's length).
 *
 *   file_checksum nblocks block_len last_block_len bpc
 * blocks 0 .. nblocks - 2 hold block_len bytes, the last one last_block_len.
 */
#include <arpa/inet.h>
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

/* The reference's loop over one block (hadooprpc.c:733-742 per packet) with
 * the drop-in crc32c(), in wire order, and the MD5 over it on the host. */
static void host_block_md5(const uint8_t *data, const crc32c_packet *pk, size_t np, uint64_t nsums, uint8_t md5[16]) {
    uint32_t *sums = malloc((nsums + 1) * 4);
    for (size_t p = 0; p < np; ++p)
        for (uint64_t o = 0, k = pk[p].out_idx; o < pk[p].len; o += pk[p].bpc, ++k) {
            const uint64_t c = pk[p].len - o < pk[p].bpc ? pk[p].len - o : pk[p].bpc;
            sums[k] = htonl(crc32c(0, data + pk[p].payload_off + o, c));
        }
    crc32c_block_md5(sums, nsums, CRC32C_BIG_ENDIAN, md5);
    free(sums);
}

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s nblocks block_len last_block_len bpc\n", argv[0]);
        return 2;
    }
    const size_t nblocks = (size_t)strtoull(argv[1], NULL, 0);
    const uint64_t block_len = strtoull(argv[2], NULL, 0), last_len = strtoull(argv[3], NULL, 0);
    const uint32_t bpc = (uint32_t)strtoul(argv[4], NULL, 0);
    if (!nblocks || !bpc) {
        fprintf(stderr, "nblocks and bpc must be positive\n");
        return 2;
    }
    const size_t nwhole = block_len == last_len ? nblocks : nblocks - 1; /* blocks of the first plan */
    const uint64_t maxlen = block_len > last_len ? block_len : last_len;

    /* 1. the blocks, on the host (for the check) and in device memory */
    uint8_t **host = calloc(nblocks, sizeof *host);
    const void **d_blocks = calloc(nblocks, sizeof *d_blocks);
    for (size_t i = 0; i < nblocks; ++i) {
        const uint64_t len = i < nwhole ? block_len : last_len;
        host[i] = malloc(len + 1);
        fill_block(host[i], len, 0x9E3779B97F4A7C15ull + i);
        void *d = NULL;
        HIP_OK(hipMalloc(&d, len + 16));
        HIP_OK(hipMemcpy(d, host[i], len, hipMemcpyHostToDevice));
        d_blocks[i] = d;
    }

    crc32c_ctx *ctx = NULL;
    int rc = crc32c_ctx_create(0, &ctx);
    CHECK(rc == 0, "ctx_create: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;

    /* 2. one plan per block shape, checksums in wire order */
    crc32c_packet *pk[2] = {NULL, NULL};
    size_t npk[2] = {0, 0};
    uint64_t nsums[2] = {0, 0};
    crc32c_plan *plan[2] = {NULL, NULL};
    npk[0] = block_packets(nwhole ? block_len : last_len, bpc, &pk[0], &nsums[0]);
    npk[1] = block_packets(last_len, bpc, &pk[1], &nsums[1]);
    for (int s = 0; s < 2; ++s) {
        rc = crc32c_plan_create(ctx, pk[s], npk[s], CRC32C_BIG_ENDIAN, &plan[s]);
        CHECK(rc == 0, "plan_create: %d (%s)", rc, crc32c_last_error());
        if (rc) return 1;
        CHECK(crc32c_plan_nchecksums(plan[s]) == nsums[s], "nchecksums %" PRIu64 " vs %" PRIu64,
              crc32c_plan_nchecksums(plan[s]), nsums[s]);
    }

    /* per-block checksum arrays and the digests, in device memory */
    const uint64_t maxsums = crc32c_nchunks(maxlen, bpc) + maxlen / 65536 + 2;
    uint32_t **d_sums = calloc(nblocks, sizeof *d_sums);
    for (size_t i = 0; i < nblocks; ++i) HIP_OK(hipMalloc((void **)&d_sums[i], maxsums * 4));
    uint8_t *d_md5 = NULL;
    HIP_OK(hipMalloc((void **)&d_md5, 16 * nblocks));
    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));

    /* 3. checksums, then their MD5s, on one stream */
    rc = crc32c_plan_exec_blocks_md5(plan[0], d_blocks, d_sums, nwhole, d_md5, stream);
    CHECK(rc == 0, "plan_exec_blocks_md5: %d (%s)", rc, crc32c_last_error());
    if (nwhole < nblocks) {
        rc = crc32c_plan_exec_blocks_md5(plan[1], d_blocks + nwhole, d_sums + nwhole, 1, d_md5 + 16 * nwhole, stream);
        CHECK(rc == 0, "plan_exec_blocks_md5 (last block): %d (%s)", rc, crc32c_last_error());
    }

    /* 4. the digests back; 5. the file checksum */
    uint8_t *md5s = malloc(16 * nblocks);
    HIP_OK(hipMemcpyAsync(md5s, d_md5, 16 * nblocks, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    uint8_t file_md5[16];
    crc32c_file_md5(md5s, nblocks, file_md5);

    /* 6. every block digest against the host loop */
    for (size_t i = 0; i < nblocks; ++i) {
        const int s = i < nwhole ? 0 : 1;
        uint8_t want[16];
        host_block_md5(host[i], pk[s], npk[s], nsums[s], want);
        CHECK(memcmp(want, md5s + 16 * i, 16) == 0, "block %zu: digest differs from crc32c_block_md5 over crc32c()", i);
    }

    /* 7. */
    char hex[33];
    for (int i = 0; i < 16; ++i) snprintf(hex + 2 * i, 3, "%02x", file_md5[i]);
    printf("%s: %s\n", fails ? "FAILED" : "ok", hex);

    for (int s = 0; s < 2; ++s) {
        crc32c_plan_destroy(plan[s]);
        free(pk[s]);
    }
    HIP_OK(hipStreamDestroy(stream));
    crc32c_ctx_destroy(ctx);
    for (size_t i = 0; i < nblocks; ++i) {
        HIP_OK(hipFree((void *)d_blocks[i]));
        HIP_OK(hipFree(d_sums[i]));
        free(host[i]);
    }
    HIP_OK(hipFree(d_md5));
    free(md5s);
    free(d_sums);
    free(d_blocks);
    free(host);
    return fails ? 1 : 0;
}
