/* striped_group.c -- one RS-6-3 striped block group of an erasure-coded file
 * handled from C through libhdfs_crc32c.so with its bytes in device memory
 * ("Erasure-coded files"):
 *   1. the group's bytes are filled on the host in file order and copied to
 *      the device;
 *   2. write side: hdfs_ec_encode_striped_dev computes the three parity blocks
 *      of every stripe in one launch; the six data blocks are checksummed
 *      where they lie in the file-order buffer (hdfs_ec_block_packets plans)
 *      and the three parity blocks with one plan of contiguous packets -- all
 *      on one stream, nothing copied back in between;
 *   3. the internal blocks as the DataNodes hold them (each contiguous) are
 *      gathered on the device; data blocks 1 and 4 and parity block 1 are
 *      dropped;
 *   4. read side: hdfs_ec_decode_matrix over the six survivors, then ONE
 *      hdfs_ec_apply_dev rebuilds the three lost blocks;
 *   5. crc32c_plan_verify checks each rebuilt block against the checksums
 *      stored in step 2; the rebuilt bytes are also compared with the
 *      originals and the parity with hdfs_ec_apply on the host;
 *   6. "ok: <crc32c of parity block 0 as 8 hex digits>".
 *
 * Fill: the xorshift64 (13, 7, 17) stream seeded with 0x9E3779B97F4A7C15, each
 * state after the step emitted as 8 little-endian bytes.  Packets of `cell`
 * bytes at most 65536 (the cell must be a multiple of 512), 512-byte chunks.
 *
 *   striped_group group_len cell
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "hdfs_crc32c.h"

enum { K = 6, M = 3, N = K + M, BPC = 512 };

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

/* A plan over the contiguous packets of a block of blen bytes (blen > 0). */
static crc32c_plan *contiguous_plan(crc32c_ctx *ctx, uint64_t blen, uint32_t packetsize) {
    const uint64_t np = crc32c_packetize(blen, 0, packetsize, BPC, NULL, 0) - 1; /* without the final empty packet */
    crc32c_packet *pk = malloc(np * sizeof *pk);
    for (uint64_t p = 0; p < np; ++p) {
        const uint64_t off = p * packetsize;
        pk[p].payload_off = off;
        pk[p].out_idx = off / BPC;
        pk[p].len = (uint32_t)(blen - off < packetsize ? blen - off : packetsize);
        pk[p].bpc = BPC;
    }
    crc32c_plan *plan = NULL;
    const int rc = crc32c_plan_create(ctx, pk, (size_t)np, 0, &plan);
    CHECK(rc == 0, "plan_create: %d (%s)", rc, crc32c_last_error());
    free(pk);
    return plan;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s group_len cell\n", argv[0]);
        return 2;
    }
    const uint64_t len = strtoull(argv[1], NULL, 0), cell = strtoull(argv[2], NULL, 0);
    if (!len || !cell || cell % BPC) {
        fprintf(stderr, "group_len must be positive and cell a positive multiple of %d\n", BPC);
        return 2;
    }
    const uint32_t packetsize = (uint32_t)(cell < 65536 ? cell : 65536);
    if (cell % packetsize) {
        fprintf(stderr, "a cell above 65536 must be a multiple of 65536\n");
        return 2;
    }

    /* 1. */
    uint8_t *file = malloc(len);
    fill_block(file, len, 0x9E3779B97F4A7C15ull);
    uint64_t blen[N];
    int rc = hdfs_ec_group_layout(len, K, M, cell, blen);
    CHECK(rc == 0, "group_layout: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;
    const uint64_t plen = blen[0], nsums = crc32c_nchunks(plen, BPC);
    uint8_t *d_file = NULL, *d_blk[N], *d_new[3];
    uint32_t *d_sums[N], *d_result = NULL;
    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_OK(hipMalloc((void **)&d_file, len + 16));
    HIP_OK(hipMemcpy(d_file, file, len, hipMemcpyHostToDevice));
    for (int u = 0; u < N; ++u) {
        HIP_OK(hipMalloc((void **)&d_blk[u], plen + 16));
        HIP_OK(hipMemsetAsync(d_blk[u], 0, plen + 16, stream)); /* (ordered before everything else on the stream) */
        HIP_OK(hipMalloc((void **)&d_sums[u], 4 * nsums));
    }
    for (int i = 0; i < 3; ++i) HIP_OK(hipMalloc((void **)&d_new[i], plen + 16));
    HIP_OK(hipMalloc((void **)&d_result, 8 * 3));

    crc32c_ctx *ctx = NULL;
    rc = crc32c_ctx_create(0, &ctx);
    CHECK(rc == 0, "ctx_create: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;

    /* 2. write side: parity, then the checksums of all nine internal blocks */
    hdfs_ec_matrix enc;
    rc = hdfs_ec_encode_matrix(HDFS_EC_RS, K, M, &enc);
    CHECK(rc == 0, "encode_matrix: %d (%s)", rc, crc32c_last_error());
    void *parity[M];
    for (int r = 0; r < M; ++r) parity[r] = d_blk[K + r];
    rc = hdfs_ec_encode_striped_dev(ctx, &enc, d_file, len, cell, parity, stream);
    CHECK(rc == 0, "encode_striped_dev: %d (%s)", rc, crc32c_last_error());
    crc32c_plan *data_plan[K] = {NULL}, *block_plan[N] = {NULL};
    for (uint32_t b = 0; b < K; ++b) {
        if (!blen[b]) continue;
        const int64_t np = hdfs_ec_block_packets(len, K, cell, b, packetsize, BPC, 0, NULL, 0);
        CHECK(np > 0, "block_packets: %" PRId64 " (%s)", np, crc32c_last_error());
        if (np <= 0) return 1;
        crc32c_packet *pk = malloc((size_t)np * sizeof *pk);
        hdfs_ec_block_packets(len, K, cell, b, packetsize, BPC, 0, pk, (size_t)np);
        rc = crc32c_plan_create(ctx, pk, (size_t)np, 0, &data_plan[b]);
        CHECK(rc == 0, "plan_create (data block %u): %d (%s)", b, rc, crc32c_last_error());
        free(pk);
        if (rc) return 1;
        rc = crc32c_plan_exec(data_plan[b], d_file, d_sums[b], stream);
        CHECK(rc == 0, "plan_exec (data block %u): %d (%s)", b, rc, crc32c_last_error());
    }
    /* contiguous plans by block length: the parity blocks' and the rebuilt blocks' */
    for (int u = 0; u < N; ++u) {
        if (!blen[u]) continue;
        for (int v = 0; v < u && !block_plan[u]; ++v)
            if (blen[v] == blen[u]) block_plan[u] = block_plan[v];
        if (!block_plan[u]) block_plan[u] = contiguous_plan(ctx, blen[u], packetsize);
        if (!block_plan[u]) return 1;
    }
    for (int r = 0; r < M; ++r) {
        rc = crc32c_plan_exec(block_plan[K + r], d_blk[K + r], d_sums[K + r], stream);
        CHECK(rc == 0, "plan_exec (parity block %d): %d (%s)", r, rc, crc32c_last_error());
    }

    /* 3. the data blocks as their DataNodes hold them: cells gathered, zeros behind */
    for (uint32_t b = 0; b < K; ++b) {
        const uint64_t rows = blen[b] / cell, tail = blen[b] % cell;
        if (rows)
            HIP_OK(hipMemcpy2DAsync(d_blk[b], cell, d_file + b * cell, K * cell, cell, rows, hipMemcpyDeviceToDevice,
                                    stream));
        if (tail)
            HIP_OK(hipMemcpyAsync(d_blk[b] + rows * cell, d_file + rows * K * cell + b * cell, tail,
                                  hipMemcpyDeviceToDevice, stream));
    }
    const uint32_t erased[3] = {1, 4, K + 1}, valid[K] = {0, 2, 3, 5, K, K + 2};

    /* 4. read side: one launch rebuilds the three lost blocks from the six survivors */
    hdfs_ec_matrix dec;
    rc = hdfs_ec_decode_matrix(HDFS_EC_RS, K, M, valid, erased, 3, &dec);
    CHECK(rc == 0, "decode_matrix: %d (%s)", rc, crc32c_last_error());
    const void *in[K];
    void *out[3];
    for (int i = 0; i < K; ++i) in[i] = d_blk[valid[i]];
    for (int i = 0; i < 3; ++i) out[i] = d_new[i];
    rc = hdfs_ec_apply_dev(ctx, &dec, in, out, plen, stream);
    CHECK(rc == 0, "apply_dev: %d (%s)", rc, crc32c_last_error());

    /* 5. the rebuilt blocks against the stored checksums */
    uint32_t result[3][2] = {{1, 0}, {1, 0}, {1, 0}};
    for (int i = 0; i < 3; ++i) {
        const uint32_t u = erased[i];
        if (!blen[u]) {
            result[i][0] = 0;
            continue;
        }
        rc = crc32c_plan_verify(block_plan[u], d_new[i], d_sums[u], d_result + 2 * i, stream);
        CHECK(rc == 0, "plan_verify (unit %u): %d (%s)", u, rc, crc32c_last_error());
        HIP_OK(hipMemcpyAsync(result[i], d_result + 2 * i, 8, hipMemcpyDeviceToHost, stream));
    }
    uint8_t *got = malloc(plen), *orig = malloc(plen), *want = malloc(plen * M), *cells = calloc(K, cell);
    uint8_t *par0 = malloc(plen);
    HIP_OK(hipMemcpyAsync(par0, d_blk[K], plen, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    /* the host's parity, stripe by stripe (short and absent cells as zeros) */
    for (uint64_t s = 0; s * cell < plen; ++s) {
        const uint64_t n = plen - s * cell < cell ? plen - s * cell : cell;
        const void *hin[K];
        void *hout[M];
        memset(cells, 0, K * cell);
        for (uint64_t j = 0; j < K; ++j) {
            const uint64_t off = (s * K + j) * cell;
            hin[j] = off < len ? cells + j * cell : NULL;
            if (off < len) memcpy(cells + j * cell, file + off, len - off < cell ? len - off : cell);
        }
        for (int r = 0; r < M; ++r) hout[r] = want + r * plen + s * cell;
        rc = hdfs_ec_apply(&enc, hin, hout, n);
        CHECK(rc == 0, "ec_apply: %d (%s)", rc, crc32c_last_error());
    }
    CHECK(memcmp(par0, want, plen) == 0, "the GPU's parity block 0 differs from the host's");
    for (int i = 0; i < 3; ++i) {
        const uint32_t u = erased[i];
        CHECK(result[i][0] == 0, "verify of rebuilt unit %u: %u mismatches", u, result[i][0]);
        HIP_OK(hipMemcpy(got, d_new[i], plen, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(orig, d_blk[u], plen, hipMemcpyDeviceToHost));
        CHECK(memcmp(got, orig, plen) == 0, "rebuilt unit %u differs from the original", u);
        if (u >= K) CHECK(memcmp(got, want + (u - K) * plen, plen) == 0, "rebuilt parity %u differs from the host's", u - K);
    }

    /* 6. */
    printf("%s: %08x\n", fails ? "FAILED" : "ok", crc32c(0, par0, plen));

    for (int u = 0; u < N; ++u) {
        int shared = 0;
        for (int v = 0; v < u; ++v) shared |= block_plan[v] == block_plan[u];
        if (block_plan[u] && !shared) crc32c_plan_destroy(block_plan[u]);
        if (u < K && data_plan[u]) crc32c_plan_destroy(data_plan[u]);
    }
    HIP_OK(hipStreamDestroy(stream));
    crc32c_ctx_destroy(ctx);
    HIP_OK(hipFree(d_file));
    for (int u = 0; u < N; ++u) {
        HIP_OK(hipFree(d_blk[u]));
        HIP_OK(hipFree(d_sums[u]));
    }
    for (int i = 0; i < 3; ++i) HIP_OK(hipFree(d_new[i]));
    HIP_OK(hipFree(d_result));
    free(got);
    free(orig);
    free(want);
    free(cells);
    free(par0);
    free(file);
    return fails ? 1 : 0;
}
