// verdicts_host.cpp -- crc32c_bitmap_verdicts_host (include/hdfs_crc32c.h
// section 6d): the host twin of the verdict kernel (crc32c_verdicts.hip),
// the path for a mismatch bitmap that is already in host memory and the CPU
// tests' counterpart of the device call.  Plain C++, no GPU; the word-level
// arithmetic is the kernel's own (verdict_cell.h).
#include <cerrno>
#include <cstdint>

#include "errors.h"
#include "hdfs_crc32c.h"
#include "verdict_cell.h"

using namespace hdfs_crc;

extern "C" int crc32c_bitmap_verdicts_host(const uint32_t *bad_bits, uint64_t nsums, uint32_t crc_per_cell,
                                           crc32c_block_verdict *verdicts) {
    if (nsums == 0) return 0;
    if (crc_per_cell == 0) return fail(-EINVAL, "crc_per_cell == 0");
    if (!bad_bits || !verdicts) return fail(-EINVAL, "bad_bits/verdicts == NULL");
    if ((uintptr_t(bad_bits) | uintptr_t(verdicts)) & 3u) return fail(-EINVAL, "bad_bits/verdicts not 4-byte aligned");
    uint64_t cell = 0;
    for (uint64_t b0 = 0; b0 < nsums; ++cell) {
        const uint64_t b1 = nsums - b0 > crc_per_cell ? b0 + crc_per_cell : nsums;
        CellAcc a;
        for (uint64_t w = b0 >> 5; w <= (b1 - 1) >> 5; ++w)
            cell_add_word(a, bad_bits[w] & cell_word_mask(w, b0, b1), w, b0);
        verdicts[cell] = cell_verdict(a, 0u);
        b0 = b1;
    }
    return 0;
}
