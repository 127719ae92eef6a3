// capture_chain_host.cpp -- the pure logic of overlapping captured execs
// (csrc/capture_chain.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
// the range-overlap predicate at its edges, the independence rule, and the
// run bookkeeping (alternating chains, the distinct-range cap).  Built and
// run by tests/test_capture_chain_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "capture_chain.h"

using namespace hdfs_crc;

static int g_failed = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                              \
        }                                                            \
    } while (0)

static ExecRanges exec_of(uint64_t payload, uint64_t payload_bytes, uint64_t out, uint64_t out_bytes) {
    ExecRanges e;
    e.payload = byte_range(payload, payload_bytes);
    e.out = byte_range(out, out_bytes);
    return e;
}

// Brute force over a small address space: the byte sets intersect.
static bool overlap_slow(uint64_t alo, uint64_t alen, uint64_t blo, uint64_t blen) {
    for (uint64_t x = alo; x < alo + alen; ++x)
        if (x >= blo && x < blo + blen) return true;
    return false;
}

int main() {
    // adjacent ranges (end == begin): no overlap, either way round
    CHECK(!ranges_overlap(byte_range(0x1000, 0x100), byte_range(0x1100, 0x100)));
    CHECK(!ranges_overlap(byte_range(0x1100, 0x100), byte_range(0x1000, 0x100)));
    // one byte of overlap
    CHECK(ranges_overlap(byte_range(0x1000, 0x101), byte_range(0x1100, 0x100)));
    CHECK(ranges_overlap(byte_range(0x1100, 0x100), byte_range(0x1000, 0x101)));
    CHECK(ranges_overlap(byte_range(0x10ff, 1), byte_range(0x1000, 0x100)));
    CHECK(!ranges_overlap(byte_range(0x1100, 1), byte_range(0x1000, 0x100)));
    // containment and identity
    CHECK(ranges_overlap(byte_range(0x1000, 0x1000), byte_range(0x1800, 4)));
    CHECK(ranges_overlap(byte_range(0x1800, 4), byte_range(0x1000, 0x1000)));
    CHECK(ranges_overlap(byte_range(0x1000, 4), byte_range(0x1000, 4)));
    // empty ranges overlap nothing, not even inside another or each other
    CHECK(!ranges_overlap(byte_range(0x1800, 0), byte_range(0x1000, 0x1000)));
    CHECK(!ranges_overlap(byte_range(0x1000, 0x1000), byte_range(0x1800, 0)));
    CHECK(!ranges_overlap(byte_range(0x1000, 0), byte_range(0x1000, 0)));
    // ranges ending at the top of the address space: no wrapped end
    const uint64_t top = UINT64_MAX;
    CHECK(byte_range(top - 15, 16).len == 16);
    CHECK(byte_range(top - 15, 64).len == 16);  // cut at the top
    CHECK(byte_range(top, 1).len == 1);
    CHECK(byte_range(top, 2).len == 1);
    CHECK(byte_range(0, top).len == top);
    CHECK(ranges_overlap(byte_range(top - 15, 16), byte_range(top, 1)));
    CHECK(ranges_overlap(byte_range(top, 1), byte_range(top - 15, 16)));
    CHECK(!ranges_overlap(byte_range(top - 15, 16), byte_range(top - 31, 16)));
    CHECK(!ranges_overlap(byte_range(top - 15, 16), byte_range(0, 16)));  // (a wrapped end would reach address 0)
    CHECK(!ranges_overlap(byte_range(0, 16), byte_range(top - 15, 64)));
    CHECK(ranges_overlap(byte_range(0, top), byte_range(top - 1, 1)));
    CHECK(!ranges_overlap(byte_range(0, top), byte_range(top, 1)));
    // rounding
    CHECK(round_up_16(0) == 0 && round_up_16(1) == 16 && round_up_16(16) == 16 && round_up_16(17) == 32);
    CHECK(round_up_16(top) == (top & ~uint64_t(15)) && round_up_16(top - 15) == (top & ~uint64_t(15)));
    // against brute force on a small space
    for (uint64_t alo = 0; alo < 12; ++alo)
        for (uint64_t alen = 0; alen < 6; ++alen)
            for (uint64_t blo = 0; blo < 12; ++blo)
                for (uint64_t blen = 0; blen < 6; ++blen)
                    CHECK(ranges_overlap(byte_range(alo, alen), byte_range(blo, blen)) ==
                          overlap_slow(alo, alen, blo, blen));

    // the rule
    const ExecRanges a = exec_of(0x10000, 0x1000, 0x20000, 0x100);
    CHECK(execs_independent(a, exec_of(0x11000, 0x1000, 0x20100, 0x100)));   // adjacent payloads and outs
    CHECK(execs_independent(a, exec_of(0x10000, 0x1000, 0x30000, 0x100)));   // the same payload, read twice
    CHECK(!execs_independent(a, exec_of(0x40000, 0x1000, 0x20000, 0x100)));  // the same out
    CHECK(!execs_independent(a, exec_of(0x40000, 0x1000, 0x200ff, 0x100)));  // outs share one byte
    CHECK(!execs_independent(a, exec_of(0x20000, 0x100, 0x30000, 0x100)));   // its payload is the other's out
    CHECK(!execs_independent(exec_of(0x20000, 0x100, 0x30000, 0x100), a));
    CHECK(!execs_independent(a, exec_of(0x200ff, 0x100, 0x30000, 0x100)));   // ... by one byte
    CHECK(execs_independent(a, exec_of(0x20100, 0x100, 0x30000, 0x100)));    // ... adjacent
    CHECK(!execs_independent(a, exec_of(0x40000, 0x100, 0x10fff, 4)));       // writes into the other's payload
    CHECK(execs_independent(a, exec_of(0x40000, 0x100, 0x11000, 4)));
    CHECK(execs_independent(a, exec_of(0x30000, 0x1000, 0x30000, 0x10)));  // (its own payload == its own out: its own affair)
    CHECK(execs_independent(exec_of(0, 0, 0x20000, 0), a));  // nothing read, nothing written

    // a run: 4 payloads into 4 outs, rotated -- every exec admitted
    ChainRun run;
    std::vector<ExecRanges> rot;
    for (uint64_t i = 0; i < 4; ++i) rot.push_back(exec_of(0x100000 * (i + 1), 0x80000, 0x900000 + 0x1000 * i, 0x1000));
    run.add(rot[0]);
    for (uint64_t k = 1; k < 64; ++k) {
        CHECK(run.next_chain() == (k & 1));
        CHECK(run.admits(rot[k % 4]));
        run.add(rot[k % 4]);
    }
    CHECK(run.nexec == 64 && run.chain[0].n == 2 && run.chain[1].n == 2);  // distinct pairs only
    // the same out on the other chain is refused; on its own chain it is ordered by the chain
    run.reset();
    run.add(rot[0]);
    CHECK(!run.admits(exec_of(0x700000, 0x100, 0x900000, 0x1000)));  // exec 1 against exec 0
    run.add(rot[1]);
    CHECK(run.admits(exec_of(0x700000, 0x100, 0x900000, 0x1000)));   // exec 2 follows exec 0 in chain 0
    CHECK(!run.admits(exec_of(0x700000, 0x100, 0x901000, 0x1000)));  // ... but not exec 1's out
    // read-after-write and write-after-read across chains
    CHECK(!run.admits(exec_of(0x901000, 0x1000, 0xa00000, 0x10)));  // exec 2 reads exec 1's out
    CHECK(!run.admits(exec_of(0x700000, 0x100, 0x200000, 0x10)));   // exec 2 writes exec 1's payload
    // the cap: chain 0 takes kChainRangesMax distinct pairs, one more starts a new run
    run.reset();
    uint64_t k = 0;
    for (; run.chain[0].n < kChainRangesMax; ++k) {
        const ExecRanges e = exec_of(0x1000000 + 0x10000 * k, 0x8000, 0x9000000 + 0x100 * k, 0x100);
        CHECK(k == 0 || run.admits(e));
        run.add(e);
    }
    CHECK(run.chain[0].n == kChainRangesMax && run.chain[1].n == kChainRangesMax - 1);
    {
        const ExecRanges e1 = exec_of(0x1000000 + 0x10000 * k, 0x8000, 0x9000000 + 0x100 * k, 0x100);
        CHECK(run.next_chain() == 1 && run.admits(e1));  // chain 1 still has room
        run.add(e1);
        ++k;
        const ExecRanges e0 = exec_of(0x1000000 + 0x10000 * k, 0x8000, 0x9000000 + 0x100 * k, 0x100);
        CHECK(run.next_chain() == 0 && !run.admits(e0));     // chain 0 is full
        CHECK(run.admits(run.chain[0].r[3]));                // a pair it already holds needs no room
        run.add(e0);                                         // (add never writes past the list)
        CHECK(run.chain[0].n == kChainRangesMax);
        run.reset();
        CHECK(run.nexec == 0 && run.chain[0].n == 0 && run.chain[1].n == 0 && run.admits(e0));
    }

    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("capture chain host run clean\n");
    return 0;
}
