// verdict_cell.h -- the word-level arithmetic of a cell's verdict
// (include/hdfs_crc32c.h section 6d), shared by the device kernel
// (crc32c_verdicts.hip) and its host twin (verdicts_host.cpp) so that both
// mask and index the same way.  A cell is the bits [b0, b1), b1 > b0, of a
// bitmap of u32 words (bit k = bit k % 32 of word k / 32).
#pragma once
#include <stdint.h>

#include "hdfs_crc32c.h"

#ifdef __HIPCC__
#define HDFS_CRC_HD __host__ __device__ __forceinline__
#else
#define HDFS_CRC_HD inline
#endif

namespace hdfs_crc {

constexpr uint32_t kVerdictNone = 0xffffffffu;
constexpr uint32_t kVerdictCountMax = 0x7fffffffu;  // (bit 31 of mismatches is CRC32C_VERIFY_OVERLAP)

// count: set bits; first / last: lowest / highest set bit counted from b0.
// The empty accumulator is the neutral element of (sum, min, max).
struct CellAcc {
    uint32_t count = 0, first = kVerdictNone, last = 0;
};

// The bits of word w that belong to the cell: the cell's first word loses
// the bits below b0, its last word the bits at and above b1 (both in one
// word for a cell inside a word).  No shift reaches 32.
HDFS_CRC_HD uint32_t cell_word_mask(uint64_t w, uint64_t b0, uint64_t b1) {
    uint32_t m = 0xffffffffu;
    if (w == (b0 >> 5)) m <<= uint32_t(b0 & 31u);
    const uint32_t r = uint32_t(b1 & 31u);
    if (r && w == ((b1 - 1) >> 5)) m &= 0xffffffffu >> (32u - r);
    return m;
}

// Word w's masked value v into the accumulator.
HDFS_CRC_HD void cell_add_word(CellAcc &a, uint32_t v, uint64_t w, uint64_t b0) {
    if (!v) return;
    a.count += uint32_t(__builtin_popcount(v));
    // (32 w + bit >= b0 for a masked bit; a cell holds fewer than 2^32 bits)
    const uint64_t base = 32u * w;
    const uint32_t lo = uint32_t(base + uint32_t(__builtin_ctz(v)) - b0);
    const uint32_t hi = uint32_t(base + (31u - uint32_t(__builtin_clz(v))) - b0);
    a.first = lo < a.first ? lo : a.first;
    a.last = hi > a.last ? hi : a.last;
}

HDFS_CRC_HD void cell_merge(CellAcc &a, uint32_t count, uint32_t first, uint32_t last) {
    a.count += count;
    a.first = first < a.first ? first : a.first;
    a.last = last > a.last ? last : a.last;
}

// The verdict of an accumulated cell; `overlap`: bit 31 or 0.
HDFS_CRC_HD crc32c_block_verdict cell_verdict(const CellAcc &a, uint32_t overlap) {
    crc32c_block_verdict v;
    v.mismatches = (a.count > kVerdictCountMax ? kVerdictCountMax : a.count) | overlap;
    v.first_bad = a.count ? a.first : kVerdictNone;
    v.last_bad = a.count ? a.last : kVerdictNone;
    v.reserved = 0;
    return v;
}

}  // namespace hdfs_crc
