// aes_host.cpp -- the host AES/CTR path (csrc/aes_ctr_host.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_aes_sanitize.py
// builds and runs it; a stand-alone program, no GPU): the NIST SP 800-38A F.5
// known answers, the counter carries, every pointer alignment, in place, and
// inputs and outputs held in exactly-sized heap blocks, so that a byte read
// or written past a buffer's end is an error here.
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

static std::vector<uint8_t> unhex(const std::string &h) {
    std::vector<uint8_t> v(h.size() / 2);
    for (size_t i = 0; i < v.size(); ++i) v[i] = uint8_t(std::stoul(h.substr(2 * i, 2), nullptr, 16));
    return v;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int main() {
    const auto iv = unhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff");
    const auto plain = unhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51");
    const struct {
        const char *key, *cipher;
    } kat[] = {{"2b7e151628aed2a6abf7158809cf4f3c", "874d6191b620e3261bef6864990db6ce9806f66b7970fdff8617187bb9fffdff"},
               {"8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b", "1abc932417521ca24f2b0459fe7e6e0b"},
               {"603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4", "601ec313775789a5b7a7f504bbf3d228"}};
    hdfs_aes_ctr ctx[3];
    for (int k = 0; k < 3; ++k) {
        const auto key = unhex(kat[k].key), want = unhex(kat[k].cipher);
        // the key in an exactly-sized block: the schedule reads no further
        uint8_t *kb = static_cast<uint8_t *>(std::malloc(key.size()));
        std::memcpy(kb, key.data(), key.size());
        CHECK(hdfs_aes_ctr_init(&ctx[k], kb, uint32_t(8 * key.size()), iv.data()) == 0, "init %d", k);
        std::free(kb);
        std::vector<uint8_t> out(plain.size());
        CHECK(hdfs_aes_ctr_xor(&ctx[k], 0, plain.data(), out.data(), out.size()) == 0, "xor %d", k);
        CHECK(std::memcmp(out.data(), want.data(), want.size()) == 0, "known answer %d", k);
    }
    {
        hdfs_aes_ctr c;
        const auto key = unhex(kat[0].key);
        const uint8_t zeros[16] = {0};
        uint8_t ks[16];
        const auto iv1 = unhex("0000000000000000ffffffffffffffff"), w1 = unhex("dc0a3bc38609c26f6f2a63a39cf7ee93");
        hdfs_aes_ctr_init(&c, key.data(), 128, iv1.data());
        hdfs_aes_ctr_xor(&c, 16, zeros, ks, 16);
        CHECK(std::memcmp(ks, w1.data(), 16) == 0, "carry into the high half");
        const auto iv2 = unhex("ffffffffffffffffffffffffffffffff"), w2 = unhex("7df76b0c1ab899b33e42f047b91b546f");
        hdfs_aes_ctr_init(&c, key.data(), 128, iv2.data());
        hdfs_aes_ctr_xor(&c, 16, zeros, ks, 16);
        CHECK(std::memcmp(ks, w2.data(), 16) == 0, "counter wrap");
        uint8_t ctr[16];
        hdfs_aes_ctr_counter(iv2.data(), UINT64_MAX, ctr);
        CHECK(ctr[15] == 0xfe && ctr[0] == 0, "counter(ff..ff, 2^64 - 1)");
        CHECK(hdfs_aes_ctr_init(&c, key.data(), 100, iv1.data()) < 0, "a 100-bit key is refused");
    }
    // Exactly-sized heap blocks at every input / output alignment: the whole
    // against byte-at-a-time calls (split invariance), then in place.
    for (int k = 0; k < 3; ++k)
        for (unsigned a_in = 0; a_in < 16; ++a_in)
            for (unsigned a_out = 0; a_out < 16; ++a_out) {
                const size_t n = size_t(rnd() % 200);
                const uint64_t s = rnd() >> (rnd() % 40);
                uint8_t *in = static_cast<uint8_t *>(std::malloc(a_in + n)) + a_in;   // ends at the block's end
                uint8_t *out = static_cast<uint8_t *>(std::malloc(a_out + n)) + a_out;
                std::vector<uint8_t> ref(n);
                for (size_t i = 0; i < n; ++i) in[i] = uint8_t(rnd());
                for (size_t i = 0; i < n; ++i) hdfs_aes_ctr_xor(&ctx[k], s + i, in + i, ref.data() + i, 1);
                CHECK(hdfs_aes_ctr_xor(&ctx[k], s, in, out, n) == 0, "xor");
                CHECK(n == 0 || std::memcmp(out, ref.data(), n) == 0, "whole vs bytes: key %d, %u/%u, n %zu", k, a_in, a_out, n);
                CHECK(hdfs_aes_ctr_xor(&ctx[k], s, in, in, n) == 0, "xor in place");
                CHECK(n == 0 || std::memcmp(in, ref.data(), n) == 0, "in place: key %d, %u, n %zu", k, a_in, n);
                std::free(in - a_in);
                std::free(out - a_out);
            }
    // the wire layout over exactly-sized arrays
    {
        const size_t np = 3;
        crc32c_packet *pk = static_cast<crc32c_packet *>(std::malloc(np * sizeof *pk));
        uint64_t *off = static_cast<uint64_t *>(std::malloc((np + 1) * sizeof *off));
        hdfs_aes_segment *seg = static_cast<hdfs_aes_segment *>(std::malloc(np * sizeof *seg));
        uint64_t *pre = static_cast<uint64_t *>(std::malloc(np * sizeof *pre));
        const uint32_t lens[3] = {65536, 700, 0};
        uint64_t pos = 0;
        for (size_t i = 0; i < np; ++i) {
            pk[i] = crc32c_packet{pos, 0, lens[i], 512};
            off[i] = 40 * i;
            pos += lens[i];
        }
        off[np] = 40 * np;
        CHECK(hdfs_aes_wire_segments(pk, np, off, 100, nullptr, nullptr, seg, pre, np) == int64_t(np), "wire_segments");
        CHECK(pre[0] == 100 && seg[0].stream_off == 140 && pre[1] == 140 + 65536 && seg[2].len == 0 &&
                  seg[2].stream_off == 100 + 120 + 65536 + 700,
              "wire layout");
        CHECK(hdfs_aes_wire_segments(pk, np, off, 100, nullptr, nullptr, seg, pre, np - 1) < 0, "cap too small");
        std::free(pk);
        std::free(off);
        std::free(seg);
        std::free(pre);
    }
    if (fails) return 1;
    std::puts("aes host sanitizer run clean");
    return 0;
}
