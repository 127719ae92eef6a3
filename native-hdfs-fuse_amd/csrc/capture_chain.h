// capture_chain.h -- the pure logic behind overlapping captured exec
// launches (crc32c_runtime.hip, capture_exec): which byte ranges two execs
// touch, whether they may run unordered, and the bookkeeping of one "run" of
// execs spread over two chains of a graph.  No HIP call: compiled and tested
// on the CPU (tests/test_capture_chain_host.py).
//
// The rule: two captured execs with no path between them in the graph must
// be independent -- their output ranges are disjoint and neither's payload
// range overlaps the other's output range.  (Payloads may overlap: both only
// read.)  Exec k of a run goes on chain k mod 2, after the run's fork set and
// the chain's previous exec; so it is ordered after execs k - 2, k - 4, ...
// by the chain itself and must be independent of every exec of the OTHER
// chain, which the per-chain lists of distinct ranges answer.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hdfs_crc {

// [lo, lo + len) in a 64-bit address space; len == 0: empty.  Kept as
// (lo, len) so a range ending at the top of the address space has no
// wrapped end to compare.
struct ByteRange {
    uint64_t lo = 0, len = 0;
};

// `bytes` bytes from `base`, cut at the top of the address space.
inline ByteRange byte_range(uint64_t base, uint64_t bytes) {
    ByteRange r;
    r.lo = base;
    const uint64_t room = ~base;  // bytes above base, less one
    r.len = bytes && bytes - 1 > room ? room + 1 : bytes;
    return r;
}

// bytes rounded up to a multiple of 16, saturating.
inline uint64_t round_up_16(uint64_t bytes) {
    return bytes > UINT64_MAX - 15 ? UINT64_MAX & ~uint64_t(15) : (bytes + 15) & ~uint64_t(15);
}

// Adjacent ranges (one's end == the other's begin) do not overlap; an empty
// range overlaps nothing.
inline bool ranges_overlap(const ByteRange &a, const ByteRange &b) {
    if (!a.len || !b.len) return false;
    return a.lo <= b.lo ? b.lo - a.lo < a.len : a.lo - b.lo < b.len;
}

// What one exec launch reads (payload) and writes (out).
struct ExecRanges {
    ByteRange payload, out;
};

inline bool same_ranges(const ExecRanges &a, const ExecRanges &b) {
    return a.payload.lo == b.payload.lo && a.payload.len == b.payload.len && a.out.lo == b.out.lo &&
           a.out.len == b.out.len;
}

inline bool execs_independent(const ExecRanges &a, const ExecRanges &b) {
    return !ranges_overlap(a.out, b.out) && !ranges_overlap(a.payload, b.out) && !ranges_overlap(b.payload, a.out);
}

// Distinct (payload, out) pairs a chain remembers; an exec that would add
// one more starts a new run (the check per exec stays a few dozen compares).
constexpr uint32_t kChainRangesMax = 16;

// One run: the execs captured since the fork, alternating over two chains.
struct ChainRun {
    struct Chain {
        ExecRanges r[kChainRangesMax];
        uint32_t n = 0;
    };
    Chain chain[2];
    uint64_t nexec = 0;

    void reset() {
        chain[0].n = chain[1].n = 0;
        nexec = 0;
    }
    // The chain the next exec goes on.
    uint32_t next_chain() const { return uint32_t(nexec & 1u); }
    // Whether the next exec may continue the run: independent of every exec
    // of the other chain, and its own chain has it already or has room.
    bool admits(const ExecRanges &e) const {
        const Chain &other = chain[1u - next_chain()], &own = chain[next_chain()];
        for (uint32_t i = 0; i < other.n; ++i)
            if (!execs_independent(e, other.r[i])) return false;
        for (uint32_t i = 0; i < own.n; ++i)
            if (same_ranges(e, own.r[i])) return true;
        return own.n < kChainRangesMax;
    }
    // Records the next exec (admits(e) held, or the run was just reset).
    void add(const ExecRanges &e) {
        Chain &own = chain[next_chain()];
        bool have = false;
        for (uint32_t i = 0; i < own.n && !have; ++i) have = same_ranges(e, own.r[i]);
        if (!have && own.n < kChainRangesMax) own.r[own.n++] = e;
        ++nexec;
    }
};

}  // namespace hdfs_crc
