// aes_ctr.h -- the one definition of AES/CTR/NoPadding the host path
// (aes_ctr_host.cpp) and the kernel (aes_ctr.hip) share (include/hdfs_crc32c.h
// section 7): S-box and T-table generation, the key schedule and the 128-bit
// counter add.  Everything here is arithmetic (FIPS 197): no table is typed
// in, so the kernel can build its LDS table from nothing.
//
// Conventions: a 16-byte AES block is four big-endian words (column c = bytes
// 4c .. 4c+3, byte 4c in bits 31..24), round keys are stored the same way
// (hdfs_aes_ctr.rk[4 r + c]), and T0[x] = (2 S[x], S[x], S[x], 3 S[x]) from
// bits 31..24 down to 7..0.  The other three round tables are T0 rotated right
// by 8, 16 and 24 bits, and S[x] is bits 15..8 (or 23..16) of T0[x].
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HDFS_AES_HD __host__ __device__
#else
#define HDFS_AES_HD
#endif

namespace hdfs_aes {

// x * 2 in GF(2^8) mod x^8 + x^4 + x^3 + x + 1 (x < 256).
constexpr HDFS_AES_HD uint32_t xtime(uint32_t x) { return ((x << 1) ^ ((x >> 7) * 0x11bu)) & 0xffu; }

constexpr HDFS_AES_HD uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i) {
        r ^= (b & 1u) ? a : 0u;
        a = xtime(a);
        b >>= 1;
    }
    return r;
}

// FIPS 197 section 5.1.1: the multiplicative inverse (x^254; 0 -> 0), then the
// affine map b ^ rotl(b, 1) ^ rotl(b, 2) ^ rotl(b, 3) ^ rotl(b, 4) ^ 0x63.
constexpr HDFS_AES_HD uint32_t sbox(uint32_t x) {
    uint32_t p = gf_mul(x, x), inv = p;  // x^2
    for (int i = 0; i < 6; ++i) {        // * x^4 * x^8 ... * x^128 = x^254
        p = gf_mul(p, p);
        inv = gf_mul(inv, p);
    }
    const uint32_t d = inv | (inv << 8);  // (rotations of a byte)
    return (inv ^ (d >> 7) ^ (d >> 6) ^ (d >> 5) ^ (d >> 4) ^ 0x63u) & 0xffu;
}

constexpr HDFS_AES_HD uint32_t te0(uint32_t x) {
    const uint32_t s = sbox(x), s2 = xtime(s);
    return (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
}

constexpr HDFS_AES_HD uint32_t ror32(uint32_t v, int n) { return (v >> n) | (v << (32 - n)); }

// ctr(n): the 128-bit big-endian value (hi, lo) plus n, carry through all 16
// bytes, wrapping mod 2^128 (Hadoop's AesCtrCryptoCodec.calculateIV).
HDFS_AES_HD inline void ctr_add(uint64_t hi, uint64_t lo, uint64_t n, uint64_t *ohi, uint64_t *olo) {
    const uint64_t l = lo + n;
    *olo = l;
    *ohi = hi + (l < lo ? 1u : 0u);
}

inline uint64_t load_be64(const uint8_t *p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return v;
}
inline void store_be64(uint8_t *p, uint64_t v) {
    for (int i = 7; i >= 0; --i, v >>= 8) p[i] = uint8_t(v);
}

// The tables of the host path, computed at compile time.
struct Tables {
    uint8_t s[256];
    uint32_t te[4][256];
    constexpr Tables() : s{}, te{} {
        for (uint32_t x = 0; x < 256; ++x) {
            const uint32_t t = te0(x);
            s[x] = uint8_t(t >> 8);
            te[0][x] = t;
            te[1][x] = ror32(t, 8);
            te[2][x] = ror32(t, 16);
            te[3][x] = ror32(t, 24);
        }
    }
};

// FIPS 197 section 5.2: key_bits / 32 key words expanded to 4 (rounds + 1)
// round-key words.  Returns the rounds (10, 12, 14), 0 for another key size.
inline uint32_t expand_key(const uint8_t *s, const uint8_t *key, uint32_t key_bits, uint32_t rk[60]) {
    if (key_bits != 128 && key_bits != 192 && key_bits != 256) return 0;
    const uint32_t nk = key_bits / 32, rounds = nk + 6, total = 4 * (rounds + 1);
    for (uint32_t i = 0; i < nk; ++i)
        rk[i] = uint32_t(key[4 * i]) << 24 | uint32_t(key[4 * i + 1]) << 16 | uint32_t(key[4 * i + 2]) << 8 | key[4 * i + 3];
    uint32_t rcon = 1;
    for (uint32_t i = nk; i < total; ++i) {
        uint32_t t = rk[i - 1];
        if (i % nk == 0) {
            t = (t << 8) | (t >> 24);
            t = uint32_t(s[t >> 24]) << 24 | uint32_t(s[(t >> 16) & 255]) << 16 | uint32_t(s[(t >> 8) & 255]) << 8 | s[t & 255];
            t ^= rcon << 24;
            rcon = xtime(rcon);
        } else if (nk > 6 && i % nk == 4) {
            t = uint32_t(s[t >> 24]) << 24 | uint32_t(s[(t >> 16) & 255]) << 16 | uint32_t(s[(t >> 8) & 255]) << 8 | s[t & 255];
        }
        rk[i] = rk[i - nk] ^ t;
    }
    for (uint32_t i = total; i < 60; ++i) rk[i] = 0;
    return rounds;
}

}  // namespace hdfs_aes
