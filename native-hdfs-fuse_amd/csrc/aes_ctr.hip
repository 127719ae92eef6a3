// aes_ctr.hip -- AES/CTR/NoPadding over device-resident bytes
// (include/hdfs_crc32c.h section 7): the packets of an encrypted transfer and
// the blocks of an encryption-zone file, XOR-ed with the keystream where they
// lie instead of being copied back to the host.
//
// Table.  One T-table (aes_ctr.h: T0[x] = (2 S, S, S, 3 S)) in LDS; the other
// three round tables are T0 rotated, and the last round takes S from bits
// 15..8 / 23..16 of the same entry.  ds_read_b32 serves 32 lanes per cycle
// over 32 banks, bank = (byte address / 4) mod 32, in the lane groups 0..31 and
// 32..63.  The table is replicated once per lane, entry x of copy c at dword
// 64 x + c: lane l reads copy l, its bank is l mod 32, and every lookup is
// conflict-free whatever the data.  64 copies instead of the 32 the banks need
// make an entry 256 bytes, so a lookup's byte address (x << 8) | 4 l is ONE
// v_perm_b32 of the state word and the lane's column -- the kernel is as much
// bound by its vector instructions as by the lookups, and 32
// copies cost a byte extract and a shift-or per lookup (measured, AES-128 over
// 256 MiB: 0.74 TB/s with 32 copies, 0.85-0.88 TB/s with 64).  64 KiB per
// workgroup, two
// workgroups of 8 waves per CU.  Each workgroup builds the table at its start
// from aes_ctr.h's generator (two threads per entry, 32 copies each, stored in
// a rotated order so that the stores spread over the banks too); nothing is
// assumed about what LDS held before.
//
// Work.  A segment (src, dst, stream_off, len) is cut at the 16-byte
// boundaries of its DESTINATION into windows; a lane takes kWinPerLane
// consecutive windows (2 or 1 in a launch too small to fill the device:
// windows_per_lane below), a wave 64 lanes' worth (a wave unit), a workgroup kWaves
// units per pass of a grid-stride loop over the launch's wave units (wave w of
// workgroup b takes units b + grid (w + kWaves i): few units still spread
// over every CU).  A window whose
// 16 bytes all belong to the segment is written with one 16-byte store; the
// first and last window of a segment off a boundary are written byte by byte,
// their bytes inside [dst, dst + len) only.
//   Keystream: with a = dst % 16 the window's byte j is stream byte
// stream_off - a + 16 w + j, i.e. keystream blocks B + w and (phase != 0 only)
// B + w + 1 shifted by phase = (stream_off - a) % 16 bytes.  Consecutive
// windows share those blocks, so a lane encrypts 4 counters for 4 windows
// (5 when phase != 0).  Counters are ctr(n) = IV + n with the full 128-bit
// carry, per lane.
//   Source: read as aligned 16-byte chunks of the source and funnel-shifted by
// (src - a) % 16 bytes (the plan kernel's shifted loads); a chunk is loaded
// only when it holds a byte of the segment, so nothing is read before the
// 16-byte boundary at or below src or past the one after its last byte.
//   dst == src: every lane then reads exactly the windows it writes.
//
// Round keys, IV and the segment references ride in the kernel arguments
// (uniform: scalar registers); a launch needs nothing built or uploaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>

#include "aes_ctr.h"
#include "hdfs_crc32c.h"
#include "hdfs_crc32c_debug.h"
#include "runtime_internal.h"

namespace hdfs_crc {
namespace {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kWaves = 8;
constexpr uint32_t kThreads = kLanes * kWaves;
constexpr uint32_t kWinPerLane = 4;                       // 16-byte windows per lane (small launches: 2 or 1)
constexpr uint32_t kCopies = 64;                          // table copies: one per lane
constexpr uint32_t kWgPerCu = 2;                          // 160 KiB / 64 KiB
constexpr uint32_t kListCap = HDFS_AES_LIST_MAX_SEGMENTS;

struct AesKey {
    uint32_t rk[60];
    uint64_t iv_hi, iv_lo;  // the IV as a 128-bit big-endian number
};

struct AesStrided {
    AesKey k;
    uint64_t src, dst;  // device addresses
    uint64_t seg_len, src_stride, dst_stride, so0, so_stride;
    uint64_t units_per_seg;  // wave units per segment
    uint64_t total;          // wave units of the launch
    uint32_t wpl;            // windows per lane (windows_per_lane)
};

struct AesList {
    AesKey k;
    uint64_t src[kListCap], dst[kListCap], so[kListCap], len[kListCap];
    uint64_t first[kListCap + 1];  // first[i]: wave units before segment i; first[n] = total
    uint32_t wpl;                  // windows per lane (windows_per_lane)
};

// (global loads and stores, not flat ones)
typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) U32x4 *GlobalConstU4;
typedef __attribute__((address_space(1))) U32x4 *GlobalU4;
typedef __attribute__((address_space(1))) uint8_t *GlobalU8;

__device__ __forceinline__ uint32_t ror(uint32_t v, uint32_t n) { return __builtin_rotateright32(v, n); }

// T0[byte kByte of s] from the lane's copy: the entry's byte address is
// (x << 8) | col, col = 4 lane, which one v_perm_b32 assembles from s and col
// (selector bytes: 0 = col's byte 0, 4 + kByte = that byte of s, 0x0c = zero).
template <int kByte>
__device__ __forceinline__ uint32_t te_at(const uint32_t *te, uint32_t col, uint32_t s) {
    const uint32_t a = __builtin_amdgcn_perm(s, col, 0x0c0c0000u | uint32_t(4 + kByte) << 8);
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(te) + a);
}

// AES_K of the counter (hi, lo) as four little-endian memory words (keystream
// bytes 0..3 in word 0, byte 0 lowest).  te: the table (entry x of copy c at
// te[64 x + c]); col: 4 lane, the byte offset of the lane's copy in an entry.
template <int kRounds>
__device__ __forceinline__ void aes_block(const AesKey &k, const uint32_t *te, uint32_t col, uint64_t hi, uint64_t lo,
                                          uint32_t (&o)[4]) {
    const uint32_t *rk = k.rk;
    uint32_t s0 = uint32_t(hi >> 32) ^ rk[0], s1 = uint32_t(hi) ^ rk[1], s2 = uint32_t(lo >> 32) ^ rk[2],
             s3 = uint32_t(lo) ^ rk[3];
#define HDFS_AES_T(kByte, w) te_at<kByte>(te, col, w)
#pragma unroll
    for (int r = 1; r < kRounds; ++r) {
        const uint32_t t0 = HDFS_AES_T(3, s0) ^ ror(HDFS_AES_T(2, s1), 8) ^ ror(HDFS_AES_T(1, s2), 16) ^
                            ror(HDFS_AES_T(0, s3), 24) ^ rk[4 * r];
        const uint32_t t1 = HDFS_AES_T(3, s1) ^ ror(HDFS_AES_T(2, s2), 8) ^ ror(HDFS_AES_T(1, s3), 16) ^
                            ror(HDFS_AES_T(0, s0), 24) ^ rk[4 * r + 1];
        const uint32_t t2 = HDFS_AES_T(3, s2) ^ ror(HDFS_AES_T(2, s3), 8) ^ ror(HDFS_AES_T(1, s0), 16) ^
                            ror(HDFS_AES_T(0, s1), 24) ^ rk[4 * r + 2];
        const uint32_t t3 = HDFS_AES_T(3, s3) ^ ror(HDFS_AES_T(2, s0), 8) ^ ror(HDFS_AES_T(1, s1), 16) ^
                            ror(HDFS_AES_T(0, s2), 24) ^ rk[4 * r + 3];
        s0 = t0, s1 = t1, s2 = t2, s3 = t3;
    }
    // last round: SubBytes + ShiftRows only; S[x] = bits 23..16 = bits 15..8 of T0[x]
    const uint32_t *lk = rk + 4 * kRounds;
    const uint32_t t0 = ((HDFS_AES_T(3, s0) & 0x00ff0000u) << 8 | (HDFS_AES_T(2, s1) & 0x00ff0000u) |
                         (HDFS_AES_T(1, s2) & 0x0000ff00u) | ((HDFS_AES_T(0, s3) >> 8) & 255u)) ^ lk[0];
    const uint32_t t1 = ((HDFS_AES_T(3, s1) & 0x00ff0000u) << 8 | (HDFS_AES_T(2, s2) & 0x00ff0000u) |
                         (HDFS_AES_T(1, s3) & 0x0000ff00u) | ((HDFS_AES_T(0, s0) >> 8) & 255u)) ^ lk[1];
    const uint32_t t2 = ((HDFS_AES_T(3, s2) & 0x00ff0000u) << 8 | (HDFS_AES_T(2, s3) & 0x00ff0000u) |
                         (HDFS_AES_T(1, s0) & 0x0000ff00u) | ((HDFS_AES_T(0, s1) >> 8) & 255u)) ^ lk[2];
    const uint32_t t3 = ((HDFS_AES_T(3, s3) & 0x00ff0000u) << 8 | (HDFS_AES_T(2, s0) & 0x00ff0000u) |
                         (HDFS_AES_T(1, s1) & 0x0000ff00u) | ((HDFS_AES_T(0, s2) >> 8) & 255u)) ^ lk[3];
#undef HDFS_AES_T
    o[0] = __builtin_bswap32(t0);
    o[1] = __builtin_bswap32(t1);
    o[2] = __builtin_bswap32(t2);
    o[3] = __builtin_bswap32(t3);
}

// Bytes off .. off + 15 of the 32 bytes (cur, next), as four memory words
// (off in 0..15; next is not looked at for off == 0).
__device__ __forceinline__ void shift16(const uint32_t (&cur)[4], const uint32_t (&next)[4], uint32_t off,
                                        uint32_t (&o)[4]) {
    // Whole words first (8, then 4 bytes), as selects between values: `off` is
    // uniform, and no array is indexed by it.
    const uint32_t e0 = cur[0], e1 = cur[1], e2 = cur[2], e3 = cur[3], e4 = next[0], e5 = next[1], e6 = next[2],
                   e7 = next[3];
    const bool w2 = (off & 8u) != 0, w1 = (off & 4u) != 0;
    const uint32_t y0 = w2 ? e2 : e0, y1 = w2 ? e3 : e1, y2 = w2 ? e4 : e2, y3 = w2 ? e5 : e3, y4 = w2 ? e6 : e4,
                   y5 = w2 ? e7 : e5;
    const uint32_t x0 = w1 ? y1 : y0, x1 = w1 ? y2 : y1, x2 = w1 ? y3 : y2, x3 = w1 ? y4 : y3, x4 = w1 ? y5 : y4;
    const uint32_t bits = (off & 3u) * 8u;
    o[0] = __builtin_amdgcn_alignbit(x1, x0, bits);
    o[1] = __builtin_amdgcn_alignbit(x2, x1, bits);
    o[2] = __builtin_amdgcn_alignbit(x3, x2, bits);
    o[3] = __builtin_amdgcn_alignbit(x4, x3, bits);
}

// The aligned 16-byte chunk at address a, or zeros when it holds no byte of
// [src, src + len) (then it is not read).
__device__ __forceinline__ void load_chunk(uint64_t a, uint64_t src, uint64_t len, bool wanted, uint32_t (&d)[4]) {
    U32x4 v = {0, 0, 0, 0};
    if (wanted && a + 16 > src && a < src + len) v = *reinterpret_cast<GlobalConstU4>(a);
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
}

// One wave unit: windows [64 wpl unit, 64 wpl (unit + 1)) of the segment, wpl
// consecutive ones per lane.
template <int kRounds>
__device__ __forceinline__ void wave_unit(const AesKey &k, const uint32_t *te, uint64_t src, uint64_t dst, uint64_t so,
                                          uint64_t len, uint64_t unit, uint32_t lane, uint32_t wpl) {
    const uint32_t a = uint32_t(dst) & 15u;
    const uint64_t end = a + len;  // bytes from the destination's boundary to the segment's end
    const uint64_t w0 = (unit * kLanes + lane) * wpl;
    if (w0 * 16 >= end) return;
    const uint64_t d0 = dst - a;
    const uint32_t ph = uint32_t(so - a) & 15u;          // keystream phase of the windows
    const uint64_t b0 = (so >= a ? (so - a) >> 4 : ~0ull) + w0;  // (block -1: no byte of it is used)
    const uint32_t sa = uint32_t(src - a) & 15u;         // source phase of the windows
    const uint64_t s0 = src - a - sa + w0 * 16;          // the lane's first aligned source chunk

    uint32_t kc[4] = {0, 0, 0, 0}, kn[4] = {0, 0, 0, 0}, dc[4], dn[4];
    load_chunk(s0, src, len, true, dc);
    // Step m = -1 encrypts the first counter; step m >= 0 loads chunk m + 1 and
    // encrypts counter m + 1 where window m (phase != 0) or window m + 1 needs
    // it, then emits window m.  One copy of the cipher's code.
#pragma unroll 1
    for (int m = -1; m < int(wpl); ++m) {
        const uint64_t wb = (w0 + uint64_t(m + 1)) * 16;  // window m + 1's first byte from d0
        // (chunk m + 1: window m's spill when the source is off phase, and window m + 1's own bytes)
        if (m >= 0) load_chunk(s0 + uint64_t(m + 1) * 16, src, len, sa != 0 || m + 1 < int(wpl), dn);
        if (m < 0 || ph != 0 || (m + 1 < int(wpl) && wb < end)) {
            uint64_t hi, lo;
            hdfs_aes::ctr_add(k.iv_hi, k.iv_lo, b0 + uint64_t(m + 1), &hi, &lo);
            aes_block<kRounds>(k, te, 4 * lane, hi, lo, kn);
        }
        if (m >= 0) {
            const uint64_t base = wb - 16;  // window m's first byte from d0 (< end)
            uint32_t ks[4], in[4];
            shift16(kc, kn, ph, ks);
            shift16(dc, dn, sa, in);
            const uint32_t o[4] = {in[0] ^ ks[0], in[1] ^ ks[1], in[2] ^ ks[2], in[3] ^ ks[3]};
            const uint32_t lo_b = base == 0 ? a : 0u;
            const uint32_t hi_b = end - base < 16 ? uint32_t(end - base) : 16u;
            const GlobalU8 out = reinterpret_cast<GlobalU8>(d0 + base);
            if (lo_b == 0 && hi_b == 16) {
                *reinterpret_cast<GlobalU4>(d0 + base) = U32x4{o[0], o[1], o[2], o[3]};
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 16; ++j)
                    if (j >= lo_b && j < hi_b) out[j] = uint8_t(o[j >> 2] >> (8 * (j & 3u)));
            }
            if (wb >= end) break;
#pragma unroll
            for (int i = 0; i < 4; ++i) dc[i] = dn[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) kc[i] = kn[i];
    }
}

// The copies of T0 (dword kCopies x + c = T0[x]); kThreads / 256 threads share an entry's copies.
__device__ __forceinline__ void build_table(uint32_t *te) {
    constexpr uint32_t kParts = kThreads / 256, kPer = kCopies / kParts;  // threads per entry, copies per thread
    const uint32_t x = threadIdx.x & 255u, first = (threadIdx.x >> 8) * kPer;
    const uint32_t v = hdfs_aes::te0(x);
#pragma unroll 4
    for (uint32_t c = first; c < first + kPer; ++c) te[kCopies * x + ((c + x) & (kCopies - 1))] = v;
    __syncthreads();
}

template <int kRounds>
__global__ __launch_bounds__(kThreads) void hdfs_aes_ctr_strided_kernel(const AesStrided p) {
    __shared__ uint32_t te[256 * kCopies];
    build_table(te);
    const uint32_t lane = threadIdx.x & (kLanes - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    for (uint64_t g = blockIdx.x + uint64_t(gridDim.x) * wave; g < p.total; g += uint64_t(gridDim.x) * kWaves) {
        const uint64_t seg = g / p.units_per_seg, unit = g - seg * p.units_per_seg;
        wave_unit<kRounds>(p.k, te, p.src + seg * p.src_stride, p.dst + seg * p.dst_stride,
                           p.so0 + seg * p.so_stride, p.seg_len, unit, lane, p.wpl);
    }
}

template <int kRounds>
__global__ __launch_bounds__(kThreads) void hdfs_aes_ctr_list_kernel(const AesList p) {
    __shared__ uint32_t te[256 * kCopies];
    build_table(te);
    const uint32_t lane = threadIdx.x & (kLanes - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const uint64_t total = p.first[kListCap];
    uint32_t i = 0;  // (units grow with g: the scan never goes back)
    for (uint64_t g = blockIdx.x + uint64_t(gridDim.x) * wave; g < total; g += uint64_t(gridDim.x) * kWaves) {
        while (i + 1 < kListCap && g >= p.first[i + 1]) ++i;
        wave_unit<kRounds>(p.k, te, p.src[i], p.dst[i], p.so[i], p.len[i], g - p.first[i], lane, p.wpl);
    }
}

// Windows of a segment of len bytes whose destination is `a` bytes past a
// 16-byte boundary.
uint64_t windows_of(uint64_t len, uint32_t a) { return len ? (len >> 4) + (((len & 15u) + a + 15u) >> 4) : 0; }

uint64_t wave_units(uint64_t windows, uint32_t wpl) { return (windows + kLanes * wpl - 1) / (kLanes * wpl); }

// Windows per lane of a launch over `windows` windows.  A lane's windows are
// encrypted one after another, so a launch that cannot fill the device's wave
// slots with kWinPerLane windows per lane takes 2 or 1: one 4 MiB block then
// runs four waves per SIMD over one AES block each instead of one wave over
// four (measured: 15.1 against 20.3 us).  Larger launches keep kWinPerLane,
// which shares the extra AES block of a keystream phase != 0.
uint32_t windows_per_lane(uint32_t num_cu, uint64_t windows) {
    const uint64_t lanes = uint64_t(std::max(num_cu, 1u)) * kWgPerCu * kThreads;
    uint32_t wpl = 1;
    while (wpl < kWinPerLane && windows > lanes * wpl) wpl *= 2;
    return wpl;
}

uint32_t grid_for(uint32_t num_cu, uint64_t total) {
    // (wave w of workgroup b takes units b + grid (w + kWaves i): a launch of few units still
    // spreads over every CU, with fewer busy waves per workgroup)
    return uint32_t(std::min<uint64_t>(total, uint64_t(std::max(num_cu, 1u)) * kWgPerCu));
}

uint32_t cus_of(const crc32c_ctx *ctx) { return uint32_t(std::max(ctx->num_cu, 1)); }

// The sizing of one launch on num_cu CUs: what the entry points launch from and
// what crc32c_debug_aes_*_launch_info report.
struct Sizing {
    uint64_t windows;  // of the whole launch (saturated)
    uint64_t total;    // wave units of the launch
    uint32_t wpl, grid;
};

// The strided form (seg_len, nsegs > 0; d: the first destination address);
// *units_per_seg: wave units per segment.  False when the wave units of the
// launch exceed 2^64.
bool size_strided(uint32_t num_cu, uint64_t d, uint64_t seg_len, uint64_t nsegs, uint64_t dst_stride, Sizing *z,
                  uint64_t *units_per_seg) {
    // Every segment has the same destination phase when the stride keeps it;
    // otherwise a segment may spill into one more window than its length fills.
    const uint32_t a = (nsegs == 1 || (dst_stride & 15u) == 0) ? uint32_t(d & 15u) : 15u;
    const uint64_t windows = windows_of(seg_len, a);
    const bool many = __builtin_mul_overflow(nsegs, windows, &z->windows);
    if (many) z->windows = ~0ull;
    z->wpl = many ? kWinPerLane : windows_per_lane(num_cu, z->windows);
    *units_per_seg = wave_units(windows, z->wpl);
    if (__builtin_mul_overflow(nsegs, *units_per_seg, &z->total)) return false;
    z->grid = grid_for(num_cu, z->total);
    return true;
}

// One list launch over segs[0 .. n), n <= kListCap; first (kListCap + 1
// entries, or NULL): the wave units before each of the kListCap slots, the
// launch's total last.
void size_list(uint32_t num_cu, const hdfs_aes_segment *segs, uint32_t n, Sizing *z, uint64_t *first) {
    const auto windows_at = [&](uint32_t j) {
        return j < n ? windows_of(segs[j].len, uint32_t(reinterpret_cast<uintptr_t>(segs[j].dst) & 15u)) : 0;
    };
    z->windows = 0;
    for (uint32_t j = 0; j < n; ++j) z->windows += windows_at(j);
    z->wpl = windows_per_lane(num_cu, z->windows);
    z->total = 0;
    for (uint32_t j = 0; j < kListCap; ++j) {
        if (first) first[j] = z->total;
        z->total += wave_units(windows_at(j), z->wpl);
    }
    if (first) first[kListCap] = z->total;
    z->grid = grid_for(num_cu, z->total);
}

int check_key(const crc32c_ctx *ctx, const hdfs_aes_ctr *c, AesKey *k) {
    if (!ctx) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(-ENODEV, "no GPU");
        return fail(-EINVAL, "ctx == NULL");
    }
    if (!c) return fail(-EINVAL, "hdfs_aes_ctr == NULL");
    if (c->rounds != 10 && c->rounds != 12 && c->rounds != 14)
        return fail(-EINVAL, "%u rounds (hdfs_aes_ctr_init sets 10, 12 or 14)", c->rounds);
    for (int i = 0; i < 60; ++i) k->rk[i] = c->rk[i];
    k->iv_hi = hdfs_aes::load_be64(c->iv);
    k->iv_lo = hdfs_aes::load_be64(c->iv + 8);
    return 0;
}

// One segment's arguments (len > 0); `what` names it in the error text.
int check_segment(uint64_t src, uint64_t dst, uint64_t so, uint64_t len, const char *what, uint64_t idx) {
    if (!src || !dst) return fail(-EINVAL, "%s %llu: %llu bytes at NULL", what, (unsigned long long)idx, (unsigned long long)len);
    if (len > (1ull << 62)) return fail(-EINVAL, "%s %llu: more than 2^62 bytes", what, (unsigned long long)idx);
    if (so + len < so && so + len != 0)
        return fail(-EINVAL, "%s %llu: stream offset + length exceeds 2^64", what, (unsigned long long)idx);
    if (src + len < src || dst + len < dst)
        return fail(-EINVAL, "%s %llu: the address range wraps", what, (unsigned long long)idx);
    if (src != dst && src < dst + len && dst < src + len)
        return fail(-EINVAL, "%s %llu: source and destination overlap without being equal", what, (unsigned long long)idx);
    return 0;
}

template <typename P, typename K10, typename K12, typename K14>
int launch(uint32_t rounds, uint32_t grid, hipStream_t s, const P &p, K10 k10, K12 k12, K14 k14) {
    const dim3 g{grid, 1, 1}, b{kThreads, 1, 1};
    if (rounds == 10)
        hipLaunchKernelGGL(k10, g, b, 0, s, p);
    else if (rounds == 12)
        hipLaunchKernelGGL(k12, g, b, 0, s, p);
    else
        hipLaunchKernelGGL(k14, g, b, 0, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

// Loads this file's code object onto the current device (crc32c_ctx_create,
// beside preload_verdict_kernels).
hipError_t preload_aes_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&hdfs_aes_ctr_strided_kernel<10>));
}

}  // namespace hdfs_crc

using namespace hdfs_crc;

extern "C" {

void crc32c_debug_aes_geometry(crc32c_debug_aes_geom *out) {
    if (!out) return;
    out->lane_bytes = 16 * kWinPerLane;
    out->wave_bytes = 16 * kWinPerLane * kLanes;
    out->workgroup_bytes = 16 * kWinPerLane * kLanes * kWaves;
    out->list_max_segments = kListCap;
    out->lanes_per_cu = kWgPerCu * kThreads;
}

static void report(const Sizing &z, crc32c_debug_aes_launch *out) {
    out->windows = z.windows;
    out->wave_units = z.total;
    out->windows_per_lane = z.wpl;
    out->grid = z.grid;
}

int crc32c_debug_aes_strided_launch_info(uint32_t num_cu, const void *dst, uint64_t seg_len, uint64_t nsegs,
                                         uint64_t dst_stride, crc32c_debug_aes_launch *out) {
    if (num_cu == 0 || !out) return fail(-EINVAL, "crc32c_debug_aes_strided_launch_info: num_cu == 0 or out == NULL");
    Sizing z{};
    uint64_t units_per_seg;
    if (seg_len != 0 && nsegs != 0 &&
        !size_strided(num_cu, uint64_t(reinterpret_cast<uintptr_t>(dst)), seg_len, nsegs, dst_stride, &z, &units_per_seg))
        return fail(-EINVAL, "%llu segments of %llu bytes are more than one launch holds", (unsigned long long)nsegs,
                    (unsigned long long)seg_len);
    report(z, out);
    return 0;
}

int crc32c_debug_aes_list_launch_info(uint32_t num_cu, const hdfs_aes_segment *segs, size_t nsegs,
                                      crc32c_debug_aes_launch *out) {
    if (num_cu == 0 || !out) return fail(-EINVAL, "crc32c_debug_aes_list_launch_info: num_cu == 0 or out == NULL");
    if (nsegs > kListCap) return fail(-EINVAL, "%llu segments: one launch holds %u", (unsigned long long)nsegs, kListCap);
    if (nsegs != 0 && !segs) return fail(-EINVAL, "segs == NULL");
    Sizing z;
    size_list(num_cu, segs, uint32_t(nsegs), &z, nullptr);
    report(z, out);
    return 0;
}

int hdfs_aes_ctr_xor_strided_dev(crc32c_ctx *ctx, const hdfs_aes_ctr *c, const void *src, void *dst,
                                 uint64_t seg_len, uint64_t nsegs, uint64_t src_stride, uint64_t dst_stride,
                                 uint64_t stream_off0, uint64_t stream_stride, void *stream) {
    AesStrided p;
    if (int rc = check_key(ctx, c, &p.k)) return rc;
    if (seg_len == 0 || nsegs == 0) return 0;
    const uint64_t s = uint64_t(reinterpret_cast<uintptr_t>(src)), d = uint64_t(reinterpret_cast<uintptr_t>(dst));
    if (int rc = check_segment(s, d, stream_off0, seg_len, "segment", 0)) return rc;
    const uint64_t last = nsegs - 1;
    uint64_t s_last, d_last, so_last;
    if (__builtin_mul_overflow(last, src_stride, &s_last) || __builtin_add_overflow(s_last, s, &s_last) ||
        __builtin_mul_overflow(last, dst_stride, &d_last) || __builtin_add_overflow(d_last, d, &d_last))
        return fail(-EINVAL, "segment %llu: the address range wraps", (unsigned long long)last);
    if (__builtin_mul_overflow(last, stream_stride, &so_last) || __builtin_add_overflow(so_last, stream_off0, &so_last))
        return fail(-EINVAL, "segment %llu: stream offset + length exceeds 2^64", (unsigned long long)last);
    if (int rc = check_segment(s_last, d_last, so_last, seg_len, "segment", last)) return rc;
    Sizing z;
    if (!size_strided(cus_of(ctx), d, seg_len, nsegs, dst_stride, &z, &p.units_per_seg))
        return fail(-EINVAL, "%llu segments of %llu bytes are more than one launch holds", (unsigned long long)nsegs,
                    (unsigned long long)seg_len);
    p.wpl = z.wpl;
    p.total = z.total;
    p.src = s;
    p.dst = d;
    p.seg_len = seg_len;
    p.src_stride = src_stride;
    p.dst_stride = dst_stride;
    p.so0 = stream_off0;
    p.so_stride = stream_stride;
    DeviceGuard guard(ctx->device);
    return launch(c->rounds, z.grid, static_cast<hipStream_t>(stream), p, hdfs_aes_ctr_strided_kernel<10>,
                  hdfs_aes_ctr_strided_kernel<12>, hdfs_aes_ctr_strided_kernel<14>);
}

int hdfs_aes_ctr_xor_list_dev(crc32c_ctx *ctx, const hdfs_aes_ctr *c, const hdfs_aes_segment *segs, size_t nsegs,
                              void *stream) {
    AesList p;
    if (int rc = check_key(ctx, c, &p.k)) return rc;
    if (nsegs == 0) return 0;
    if (!segs) return fail(-EINVAL, "segs == NULL");
    for (size_t i = 0; i < nsegs; ++i) {
        if (segs[i].len == 0) continue;
        if (int rc = check_segment(uint64_t(reinterpret_cast<uintptr_t>(segs[i].src)),
                                   uint64_t(reinterpret_cast<uintptr_t>(segs[i].dst)), segs[i].stream_off, segs[i].len,
                                   "segment", i))
            return rc;
    }
    DeviceGuard guard(ctx->device);
    for (size_t i = 0; i < nsegs; i += kListCap) {
        const uint32_t n = uint32_t(std::min<size_t>(kListCap, nsegs - i));
        Sizing z;
        size_list(cus_of(ctx), segs + i, n, &z, p.first);
        p.wpl = z.wpl;
        for (uint32_t j = 0; j < kListCap; ++j) {
            const bool live = j < n && segs[i + j].len != 0;
            p.src[j] = live ? uint64_t(reinterpret_cast<uintptr_t>(segs[i + j].src)) : 0;
            p.dst[j] = live ? uint64_t(reinterpret_cast<uintptr_t>(segs[i + j].dst)) : 0;
            p.so[j] = live ? segs[i + j].stream_off : 0;
            p.len[j] = live ? segs[i + j].len : 0;
        }
        if (z.total == 0) continue;
        if (int rc = launch(c->rounds, z.grid, static_cast<hipStream_t>(stream), p, hdfs_aes_ctr_list_kernel<10>,
                            hdfs_aes_ctr_list_kernel<12>, hdfs_aes_ctr_list_kernel<14>))
            return rc;
    }
    return 0;
}

}  // extern "C"
