/* encrypted_block.c -- a block of an encryption-zone file handled from C
 * through libhdfs_crc32c.so with its bytes in device memory (INTEGRATION.md,
 * "Encrypted transfer and encryption zones"):
 *   1. the block's plaintext is filled on the host and copied to the device;
 *   2. hdfs_aes_ctr_init with the file's key and IV (FileEncryptionInfo); the
 *      keystream position of the block's first byte is its file offset;
 *   3. write side: hdfs_aes_ctr_xor_strided_dev (one segment) encrypts into a
 *      second device buffer, then a plan of the block's packets checksums the
 *      CIPHERTEXT (a zone file's checksums cover what the DataNode stores) and
 *      crc32c_composite_cells combines them into the block's composite CRC --
 *      all on one stream, nothing copied back in between;
 *   4. read side: crc32c_plan_verify checks the ciphertext against those
 *      checksums, then the same AES call decrypts it in place;
 *   5. the ciphertext is compared with hdfs_aes_ctr_xor on the host, the
 *      composite CRC with crc32c() over the host's ciphertext, the decrypted
 *      bytes with the plaintext;
 *   6. "ok: <composite CRC of the ciphertext as 8 hex digits>".
 *
 * Fill: the xorshift64 (13, 7, 17) stream seeded with 0x9E3779B97F4A7C15, each
 * state after the step emitted as 8 little-endian bytes.  Key: bytes 00 01 02
 * ... ; IV: bytes f0 f1 ... ff.
 *
 *   encrypted_block block_len bpc file_offset key_bits
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

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s block_len bpc file_offset key_bits\n", argv[0]);
        return 2;
    }
    const uint64_t len = strtoull(argv[1], NULL, 0), file_off = strtoull(argv[3], NULL, 0);
    const uint32_t bpc = (uint32_t)strtoul(argv[2], NULL, 0), key_bits = (uint32_t)strtoul(argv[4], NULL, 0);
    if (!len || !bpc) {
        fprintf(stderr, "block_len and bpc must be positive\n");
        return 2;
    }

    /* 1. */
    uint8_t *plain = malloc(len), *cipher = malloc(len), *back = malloc(len);
    fill_block(plain, len, 0x9E3779B97F4A7C15ull);
    void *d_plain = NULL, *d_cipher = NULL;
    HIP_OK(hipMalloc(&d_plain, len + 16));
    HIP_OK(hipMalloc(&d_cipher, len + 16));
    HIP_OK(hipMemcpy(d_plain, plain, len, hipMemcpyHostToDevice));

    /* 2. */
    uint8_t key[32], iv[16];
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)i;
    for (int i = 0; i < 16; ++i) iv[i] = (uint8_t)(0xf0 + i);
    hdfs_aes_ctr aes;
    int rc = hdfs_aes_ctr_init(&aes, key, key_bits, iv);
    CHECK(rc == 0, "aes_ctr_init: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;

    crc32c_ctx *ctx = NULL;
    rc = crc32c_ctx_create(0, &ctx);
    CHECK(rc == 0, "ctx_create: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;

    /* the block's packets (hadooprpc.c:827-857), checksums packed in packet order */
    const uint64_t np = crc32c_packetize(len, 0, 65536, bpc, NULL, 0);
    uint64_t *lens = malloc((np + 1) * sizeof *lens);
    crc32c_packet *pk = malloc((np + 1) * sizeof *pk);
    crc32c_packetize(len, 0, 65536, bpc, lens, np);
    uint64_t pos = 0, nsums = 0;
    for (uint64_t p = 0; p < np; ++p) {
        pk[p].payload_off = pos;
        pk[p].out_idx = nsums;
        pk[p].len = (uint32_t)lens[p];
        pk[p].bpc = bpc;
        pos += lens[p];
        nsums += crc32c_nchunks(lens[p], bpc);
    }
    crc32c_plan *plan = NULL;
    rc = crc32c_plan_create(ctx, pk, (size_t)np, 0, &plan);
    CHECK(rc == 0, "plan_create: %d (%s)", rc, crc32c_last_error());
    if (rc) return 1;
    uint32_t sb = 0, last_len = 0;
    rc = crc32c_plan_composite_shape(plan, &sb, &last_len);
    CHECK(rc == 0 && sb == bpc, "plan_composite_shape: %d (%s)", rc, crc32c_last_error());

    uint32_t *d_sums = NULL, *d_crc = NULL, *d_result = NULL;
    HIP_OK(hipMalloc((void **)&d_sums, 4 * nsums));
    HIP_OK(hipMalloc((void **)&d_crc, 4));
    HIP_OK(hipMalloc((void **)&d_result, 8));
    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));

    /* 3. write side: encrypt, then checksum the ciphertext */
    rc = hdfs_aes_ctr_xor_strided_dev(ctx, &aes, d_plain, d_cipher, len, 1, 0, 0, file_off, 0, stream);
    CHECK(rc == 0, "aes_ctr_xor_strided_dev (encrypt): %d (%s)", rc, crc32c_last_error());
    rc = crc32c_plan_exec(plan, d_cipher, d_sums, stream);
    CHECK(rc == 0, "plan_exec: %d (%s)", rc, crc32c_last_error());
    rc = crc32c_composite_cells(ctx, d_sums, nsums, (uint32_t)nsums, bpc, last_len, 0, d_crc, stream);
    CHECK(rc == 0, "composite_cells: %d (%s)", rc, crc32c_last_error());
    HIP_OK(hipMemcpyAsync(cipher, d_cipher, len, hipMemcpyDeviceToHost, stream));

    /* 4. read side: verify, then decrypt in place */
    rc = crc32c_plan_verify(plan, d_cipher, d_sums, d_result, stream);
    CHECK(rc == 0, "plan_verify: %d (%s)", rc, crc32c_last_error());
    rc = hdfs_aes_ctr_xor_strided_dev(ctx, &aes, d_cipher, d_cipher, len, 1, 0, 0, file_off, 0, stream);
    CHECK(rc == 0, "aes_ctr_xor_strided_dev (decrypt): %d (%s)", rc, crc32c_last_error());
    uint32_t crc = 0, result[2] = {1, 0};
    HIP_OK(hipMemcpyAsync(back, d_cipher, len, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(&crc, d_crc, 4, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(result, d_result, 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));

    /* 5. */
    uint8_t *want = malloc(len);
    rc = hdfs_aes_ctr_xor(&aes, file_off, plain, want, len);
    CHECK(rc == 0, "aes_ctr_xor: %d (%s)", rc, crc32c_last_error());
    CHECK(memcmp(cipher, want, len) == 0, "the GPU's ciphertext differs from the host's");
    CHECK(memcmp(cipher, plain, len) != 0, "the ciphertext equals the plaintext");
    CHECK(result[0] == 0, "verify of the ciphertext: %u mismatches", result[0]);
    CHECK(memcmp(back, plain, len) == 0, "decrypting did not restore the plaintext");
    const uint32_t want_crc = crc32c(0, want, len);
    CHECK(crc == want_crc, "composite %08x, crc32c() over the ciphertext %08x", crc, want_crc);

    /* 6. */
    printf("%s: %08x\n", fails ? "FAILED" : "ok", crc);

    crc32c_plan_destroy(plan);
    HIP_OK(hipStreamDestroy(stream));
    crc32c_ctx_destroy(ctx);
    HIP_OK(hipFree(d_plain));
    HIP_OK(hipFree(d_cipher));
    HIP_OK(hipFree(d_sums));
    HIP_OK(hipFree(d_crc));
    HIP_OK(hipFree(d_result));
    free(want);
    free(pk);
    free(lens);
    free(plain);
    free(cipher);
    free(back);
    return fails ? 1 : 0;
}
