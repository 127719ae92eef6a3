// ec_host.cpp -- the host erasure-coding path (csrc/ec_gf256.h,
// csrc/ec_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_ec_sanitize.py builds and runs it; a stand-alone program, no
// GPU): the stated known answers, every erasure pattern of RS(6,3), every
// pointer alignment, NULL inputs, and inputs, outputs and packet arrays held
// in exactly-sized heap blocks, so that a byte read or written past a
// buffer's end is an error here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hdfs_crc32c.h"

static int fails = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            std::fprintf(stderr, "FAIL line %d: ", __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);              \
            std::fputc('\n', stderr);                       \
            ++fails;                                        \
        }                                                   \
    } while (0)

static std::string hex(const uint8_t *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// An exactly-sized heap block of `off + n` bytes; the unit starts `off` bytes in and ends at the block's end.
static uint8_t *unit(size_t off, size_t n) { return static_cast<uint8_t *>(std::malloc(off + n ? off + n : 1)) + off; }

int main() {
    CHECK(hdfs_gf256_mul(0x53, 0xca) == 0x8f && hdfs_gf256_mul(2, 0x80) == 0x1d, "products");
    CHECK(hdfs_gf256_inv(2) == 0x8e && hdfs_gf256_inv(3) == 0xf4 && hdfs_gf256_inv(0) == 0, "inverses");
    for (unsigned a = 1; a < 256; ++a) CHECK(hdfs_gf256_mul(uint8_t(a), hdfs_gf256_inv(uint8_t(a))) == 1, "a * inv(a), a = %u", a);

    hdfs_ec_matrix enc;
    CHECK(hdfs_ec_encode_matrix(HDFS_EC_RS, 6, 3, &enc) == 0, "encode_matrix");
    CHECK(hex(enc.coef[0], 6) == "7aba47a78ef4" && hex(enc.coef[1], 6) == "ba7aa747f48e" && hex(enc.coef[2], 6) == "ad9ddd983daa",
          "the rows of P for RS(6,3)");
    CHECK(hdfs_ec_encode_matrix(HDFS_EC_RS, 17, 3, &enc) < 0 && hdfs_ec_encode_matrix(HDFS_EC_XOR, 2, 2, &enc) < 0, "refused schemes");
    CHECK(hdfs_ec_encode_matrix(HDFS_EC_RS, 6, 3, &enc) == 0, "encode_matrix");

    // the parity pins over exactly-sized units
    {
        const size_t n = 4096;
        uint8_t *u[9];
        for (int j = 0; j < 9; ++j) u[j] = unit(0, n);
        for (int j = 0; j < 6; ++j)
            for (size_t t = 0; t < n; ++t) u[j][t] = uint8_t(31 * j + 7 * t + 1);
        const void *in[6] = {u[0], u[1], u[2], u[3], u[4], u[5]};
        void *out[3] = {u[6], u[7], u[8]};
        CHECK(hdfs_ec_apply(&enc, in, out, n) == 0, "apply");
        CHECK(hex(u[6], 16) == "127eb5a56ffa1909909005dcdf764c8c", "p0 of RS(6,3)");
        CHECK(hex(u[7], 16) == "45836063ba0796601fc4d01a0a32e545", "p1 of RS(6,3)");
        CHECK(hex(u[8], 16) == "495c1c224a9e69132d8140f81611c834", "p2 of RS(6,3)");
        // every pattern of three lost units, from the first six survivors
        uint8_t *back[3] = {unit(0, n), unit(0, n), unit(0, n)};
        for (uint32_t e0 = 0; e0 < 9; ++e0)
            for (uint32_t e1 = e0 + 1; e1 < 9; ++e1)
                for (uint32_t e2 = e1 + 1; e2 < 9; ++e2) {
                    const uint32_t erased[3] = {e0, e1, e2};
                    uint32_t valid[6], nv = 0;
                    for (uint32_t v = 0; v < 9; ++v)
                        if (v != e0 && v != e1 && v != e2) valid[nv++] = v;
                    hdfs_ec_matrix dec;
                    CHECK(hdfs_ec_decode_matrix(HDFS_EC_RS, 6, 3, valid, erased, 3, &dec) == 0, "decode_matrix");
                    const void *din[6];
                    for (int i = 0; i < 6; ++i) din[i] = u[valid[i]];
                    void *dout[3] = {back[0], back[1], back[2]};
                    CHECK(hdfs_ec_apply(&dec, din, dout, n) == 0, "apply (decode)");
                    for (int i = 0; i < 3; ++i)
                        CHECK(std::memcmp(back[i], u[erased[i]], n) == 0, "pattern %u %u %u: unit %u", e0, e1, e2, erased[i]);
                }
        const uint32_t valid[6] = {0, 2, 3, 5, 6, 8}, both[1] = {2}, far[1] = {9};
        hdfs_ec_matrix dec;
        CHECK(hdfs_ec_decode_matrix(HDFS_EC_RS, 6, 3, valid, both, 1, &dec) < 0, "an index in both lists is refused");
        CHECK(hdfs_ec_decode_matrix(HDFS_EC_RS, 6, 3, valid, far, 1, &dec) < 0, "an index out of range is refused");
        for (int j = 0; j < 9; ++j) std::free(u[j]);
        for (int i = 0; i < 3; ++i) std::free(back[i]);
    }

    // Every input / output alignment, exactly-sized blocks, a NULL input in
    // turn: the whole against byte-at-a-time calls (split invariance).
    for (uint32_t k : {1u, 3u, 16u})
        for (uint32_t m : {1u, 4u})
            for (unsigned a = 0; a < 16; ++a) {
                hdfs_ec_matrix mx;
                std::memset(&mx, 0, sizeof mx);
                mx.n_in = k;
                mx.n_out = m;
                for (uint32_t r = 0; r < m; ++r)
                    for (uint32_t j = 0; j < k; ++j) mx.coef[r][j] = uint8_t(rnd());
                const size_t n = size_t(rnd() % 600);
                const uint32_t absent = uint32_t(rnd() % (k + 1));  // (k: none)
                uint8_t *in[16], *out[4], *ref[4];
                const void *inp[16];
                void *outp[4];
                for (uint32_t j = 0; j < k; ++j) {
                    in[j] = unit((a + 3 * j) % 16, n);
                    for (size_t t = 0; t < n; ++t) in[j][t] = uint8_t(rnd());
                    inp[j] = j == absent ? nullptr : in[j];
                }
                for (uint32_t r = 0; r < m; ++r) {
                    out[r] = unit((a + 5 * r + 1) % 16, n);
                    ref[r] = unit(0, n);
                    outp[r] = out[r];
                }
                for (size_t t = 0; t < n; ++t) {
                    const void *ip[16];
                    void *op[4];
                    for (uint32_t j = 0; j < k; ++j) ip[j] = inp[j] ? in[j] + t : nullptr;
                    for (uint32_t r = 0; r < m; ++r) op[r] = ref[r] + t;
                    hdfs_ec_apply(&mx, ip, op, 1);
                }
                CHECK(hdfs_ec_apply(&mx, inp, outp, n) == 0, "apply");
                for (uint32_t r = 0; r < m; ++r)
                    CHECK(n == 0 || std::memcmp(out[r], ref[r], n) == 0, "whole vs bytes: %u x %u, a %u, n %zu, row %u", k, m, a, n, r);
                for (uint32_t j = 0; j < k; ++j) std::free(in[j] - (a + 3 * j) % 16);
                for (uint32_t r = 0; r < m; ++r) {
                    std::free(out[r] - (a + 5 * r + 1) % 16);
                    std::free(ref[r]);
                }
            }

    // the layout and the packets over exactly-sized arrays
    {
        const uint64_t cell = 4096, len = 2 * 6 * cell + cell / 2;
        uint64_t *bl = static_cast<uint64_t *>(std::malloc(9 * sizeof *bl));
        CHECK(hdfs_ec_group_layout(len, 6, 3, cell, bl) == 0, "group_layout");
        CHECK(bl[0] == 2 * cell + cell / 2 && bl[1] == 2 * cell && bl[5] == 2 * cell && bl[6] == bl[0] && bl[8] == bl[0], "layout");
        const int64_t np = hdfs_ec_block_packets(len, 6, cell, 0, 2048, 512, 7, nullptr, 0);
        CHECK(np == 5, "block 0 has %lld packets", (long long)np);
        crc32c_packet *pk = static_cast<crc32c_packet *>(std::malloc(size_t(np) * sizeof *pk));
        CHECK(hdfs_ec_block_packets(len, 6, cell, 0, 2048, 512, 7, pk, size_t(np)) == np, "block_packets");
        CHECK(pk[0].payload_off == 0 && pk[1].payload_off == 2048 && pk[2].payload_off == 6 * cell && pk[4].payload_off == 12 * cell &&
                  pk[4].len == 2048 && pk[4].out_idx == 7 + 16,
              "packets of block 0");
        CHECK(hdfs_ec_block_packets(len, 6, cell, 0, 2048, 512, 7, pk, size_t(np) - 1) < 0, "cap too small");
        CHECK(hdfs_ec_block_packets(len, 6, cell, 0, 3000, 512, 7, pk, size_t(np)) < 0, "cell % packetsize");
        std::free(pk);
        std::free(bl);
    }
    if (fails) return 1;
    std::puts("ec host sanitizer run clean");
    return 0;
}
