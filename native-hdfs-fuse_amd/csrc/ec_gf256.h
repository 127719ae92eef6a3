// ec_gf256.h -- the one definition of the erasure-coding arithmetic the host
// path (ec_host.cpp) and the kernel (ec_rs.hip) share (include/hdfs_crc32c.h
// section 8): GF(2^8) mod x^8 + x^4 + x^3 + x^2 + 1 (0x11d: ISA-L's and
// Hadoop's GF256 field), the Cauchy parity matrix, matrix inversion, and the
// generator of the nibble tables both paths look bytes up in.  Everything
// here is arithmetic: no table is typed in, so the kernel can build its LDS
// tables from the matrix alone.
//
// Nibble tables.  out[r][t] = sum_j coef[r][j] * in[j][t], and
// c * b = c * (b & 15) ^ c * (b & 0xf0), so per input j two tables of 16
// entries suffice.  An entry is one dword holding the products for ALL (up to
// 4) output rows, row r in bits 8 r + 7 .. 8 r: entry e = 32 j + 16 h + n of
// the image is (coef[r][j] * (h ? n << 4 : n)) for r = 0 .. 3.  One lookup
// pair per input byte serves every output row at once; the accumulated dword
// of a byte position is that position's byte of every row.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HDFS_EC_HD __host__ __device__
#else
#define HDFS_EC_HD
#endif

namespace hdfs_ec {

constexpr uint32_t kMaxIn = 16;           // k <= 16
constexpr uint32_t kMaxOut = 4;           // m <= 4
constexpr uint32_t kEntriesPerInput = 32; // two nibble tables of 16 dwords

// a * b in GF(2^8) mod 0x11d (a, b < 256).
constexpr HDFS_EC_HD uint32_t mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i) {
        r ^= (b & 1u) ? a : 0u;
        a = ((a << 1) ^ ((a >> 7) * 0x11du)) & 0xffu;
        b >>= 1;
    }
    return r;
}

// The multiplicative inverse a^254 (0 -> 0).
constexpr HDFS_EC_HD uint32_t inv(uint32_t a) {
    uint32_t p = mul(a, a), r = p;  // a^2
    for (int i = 0; i < 6; ++i) {   // * a^4 * a^8 ... * a^128 = a^254
        p = mul(p, p);
        r = mul(r, p);
    }
    return r;
}

// Entry e (< 32 n_in) of the nibble-table image of a matrix (coef[r][j], rows
// r >= n_out count as zero).
HDFS_EC_HD inline uint32_t table_entry(const uint8_t (*coef)[kMaxIn], uint32_t n_out, uint32_t e) {
    const uint32_t j = e >> 5, n = e & 15u, x = (e & 16u) ? n << 4 : n;
    uint32_t v = 0;
    for (uint32_t r = 0; r < kMaxOut; ++r)
        if (r < n_out) v |= mul(coef[r][j], x) << (8 * r);
    return v;
}

// P[r][j] of the RS(k, m) Cauchy part (Hadoop's RSUtil.genCauchyMatrix,
// ISA-L's gf_gen_cauchy1_matrix): 1 / ((k + r) ^ j).
constexpr uint32_t cauchy(uint32_t k, uint32_t r, uint32_t j) { return inv((k + r) ^ j); }

// In-place Gauss-Jordan inverse of the n x n matrix a (n <= kMaxIn) into b;
// false when a is singular.  a is destroyed.
inline bool invert(uint8_t a[kMaxIn][kMaxIn], uint8_t b[kMaxIn][kMaxIn], uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < n; ++j) b[i][j] = i == j;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t p = c;
        while (p < n && a[p][c] == 0) ++p;
        if (p == n) return false;
        if (p != c)
            for (uint32_t j = 0; j < n; ++j) {
                const uint8_t ta = a[p][j], tb = b[p][j];
                a[p][j] = a[c][j], a[c][j] = ta;
                b[p][j] = b[c][j], b[c][j] = tb;
            }
        const uint32_t d = inv(a[c][c]);
        for (uint32_t j = 0; j < n; ++j) {
            a[c][j] = uint8_t(mul(a[c][j], d));
            b[c][j] = uint8_t(mul(b[c][j], d));
        }
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t f = a[i][c];
            if (i == c || f == 0) continue;
            for (uint32_t j = 0; j < n; ++j) {
                a[i][j] ^= uint8_t(mul(a[c][j], f));
                b[i][j] ^= uint8_t(mul(b[c][j], f));
            }
        }
    }
    return true;
}

}  // namespace hdfs_ec
