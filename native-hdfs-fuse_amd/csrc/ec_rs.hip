// ec_rs.hip -- Reed-Solomon / XOR erasure coding over device-resident bytes
// (include/hdfs_crc32c.h section 8): out[r][t] = sum_j coef[r][j] * in[j][t]
// in GF(2^8), for the parity cells of a striped block group and for the
// reconstruction of lost internal blocks.
//
// Tables.  Per input j two tables of 16 dwords, keyed by the low and the high
// nibble of a data byte (ec_gf256.h); an entry holds the products for all (up
// to 4) output rows, one per byte, so one lookup pair per data byte serves
// every output row.  32 entries per input, at most 512 per matrix.  The image
// is replicated 32 times, entry e of copy c at dword 32 e + c: lane l reads
// copy l mod 32, ds_read_b32 serves the lane groups 0..31 and 32..63 in one
// cycle each over 32 banks, bank = (byte address / 4) mod 32 = l mod 32, so
// every lookup is conflict-free whatever the data.  4 KiB of LDS per input
// (dynamic: 24 KiB for RS-6-3, 64 KiB at k = 16), so up to four workgroups of
// 8 waves share a CU: 32 resident waves instead of 16 measured 10 % faster
// (the kernel is bound by instruction issue).  A full
// 256-entry table per input would be k KiB per copy -- one lookup per byte, but
// no room for a copy per bank from k = 6 on, and none for more waves.  Each
// workgroup builds the image at its start from the matrix in the kernel
// arguments (thread e computes entry e and stores its 32 copies in a rotated
// order, so the stores spread over the banks too); nothing is assumed about
// what LDS held before.
//
// Work.  A unit (the outputs' len bytes) is cut at the 16-byte boundaries of
// OUTPUT 0 into windows; a lane takes one window, a wave 64 consecutive ones (a
// wave unit), a workgroup kWaves wave units per pass of a grid-stride loop
// over the launch's wave units (wave w of workgroup b takes units b + grid (w
// + kWaves i): few units still spread over every CU).  Per window a lane
// accumulates 16 dwords (one per byte position) over the inputs, then four
// 4 x 4 byte transposes (v_perm_b32) turn them into four words per output row.
//   Inputs: read as aligned 16-byte chunks and funnel-shifted by the input's
// phase against output 0 (the plan kernel's shifted loads); a chunk is loaded
// only when it holds a byte of the input, so nothing is read before the
// 16-byte boundary at or below an input's first byte or past the one after its
// last.  Input j + 1's chunks are requested before input j's lookups.  A NULL
// input (or a cell past the end of a short stripe) is skipped; the part of a
// window past a short cell's end is masked to zero.
//   Outputs: a full window of an output in phase with output 0 is one 16-byte
// store; an output off that phase takes the widest naturally aligned stores
// its phase allows (8, 4, 2 or 1 bytes); the first and last window of a unit
// off a boundary are written byte by byte, inside [out, out + len) only.
//
// The matrix and the unit references ride in the kernel arguments (uniform:
// scalar registers); a launch needs nothing built or uploaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>

#include "ec_gf256.h"
#include "hdfs_crc32c.h"
#include "hdfs_crc32c_debug.h"
#include "runtime_internal.h"

namespace hdfs_crc {
namespace {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kWaves = 8;
constexpr uint32_t kThreads = kLanes * kWaves;
constexpr uint32_t kCopies = 32;   // table copies: one per bank
constexpr uint32_t kLdsPerInput = hdfs_ec::kEntriesPerInput * kCopies * 4;  // 4 KiB
constexpr uint32_t kLdsPerCu = 160u << 10;
constexpr uint32_t kMaxWgPerCu = 4;  // 32 waves per CU
constexpr uint32_t kMaxIn = hdfs_ec::kMaxIn, kMaxOut = hdfs_ec::kMaxOut;
static_assert(kThreads >= kMaxIn * hdfs_ec::kEntriesPerInput, "one thread per table entry");

struct EcArgs {
    uint64_t in[kMaxIn];    // apply: device addresses of the inputs (0: zeros); striped: in[0] = src
    uint64_t out[kMaxOut];  // device addresses of the outputs
    uint8_t coef[kMaxOut][kMaxIn];
    uint32_t n_in, n_out;
    uint64_t len;              // apply: bytes per unit; striped: bytes of the block group
    uint64_t cell;             // striped
    uint64_t units_per_stripe; // striped: wave units per stripe
    uint64_t total;            // wave units of the launch
};

// (global loads and stores, not flat ones)
typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t U32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) U32x4 *GlobalConstU4;
typedef __attribute__((address_space(1))) U32x4 *GlobalU4;
typedef __attribute__((address_space(1))) U32x2 *GlobalU2;
typedef __attribute__((address_space(1))) uint32_t *GlobalU1;
typedef __attribute__((address_space(1))) uint16_t *GlobalU16;
typedef __attribute__((address_space(1))) uint8_t *GlobalU8;

// Bytes off .. off + 15 of the 32 bytes (cur, next), as four memory words
// (off in 0..15, uniform; next is not looked at for off == 0).
__device__ __forceinline__ void shift16(const U32x4 cur, const U32x4 next, uint32_t off, uint32_t (&o)[4]) {
    const uint32_t e0 = cur.x, e1 = cur.y, e2 = cur.z, e3 = cur.w, e4 = next.x, e5 = next.y, e6 = next.z, e7 = next.w;
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
__device__ __forceinline__ U32x4 load_chunk(uint64_t a, uint64_t src, uint64_t len, bool wanted) {
    U32x4 v = {0, 0, 0, 0};
    if (wanted && a + 16 > src && a < src + len) v = *reinterpret_cast<GlobalConstU4>(a);
    return v;
}

// One input of a unit: its address and its bytes (0: absent).
struct Input {
    uint64_t addr, len;
};

template <bool kStriped>
__device__ __forceinline__ Input input_of(const EcArgs &p, uint64_t stripe, uint32_t j, uint64_t ulen) {
    if (kStriped) {
        const uint64_t off = (stripe * p.n_in + j) * p.cell;  // the cell's file offset
        if (off >= p.len) return Input{0, 0};
        return Input{p.in[0] + off, p.len - off < p.cell ? p.len - off : p.cell};
    }
    return Input{p.in[j], p.in[j] ? ulen : 0};
}

// The two aligned chunks that hold a lane's window of an input.
struct Raw {
    U32x4 c0, c1;
    uint32_t sa;  // the input's phase against the windows
};

__device__ __forceinline__ Raw load_window(const Input in, uint32_t a, uint64_t wb) {
    Raw r;
    r.sa = uint32_t(in.addr - a) & 15u;
    const uint64_t s0 = in.addr - a - r.sa + wb;  // the aligned chunk of the window's first byte
    r.c0 = load_chunk(s0, in.addr, in.len, in.len != 0);
    r.c1 = load_chunk(s0 + 16, in.addr, in.len, in.len != 0 && r.sa != 0);
    return r;
}

// One wave unit: windows [64 unit, 64 (unit + 1)) of a unit (apply: the only
// one; striped: stripe `stripe`), one per lane.
template <bool kStriped>
__device__ __forceinline__ void wave_unit(const EcArgs &p, const uint32_t *tab, uint64_t stripe, uint64_t unit,
                                          uint32_t lane) {
    uint64_t ulen = p.len, ooff = 0;
    if (kStriped) {
        const uint64_t done = stripe * p.n_in * p.cell;
        ulen = p.len - done < p.cell ? p.len - done : p.cell;  // the length of the stripe's cell 0
        ooff = stripe * p.cell;
    }
    const uint64_t o0 = p.out[0] + ooff;
    const uint32_t a = uint32_t(o0) & 15u;
    const uint64_t end = a + ulen;  // bytes from output 0's boundary to the unit's end
    const uint64_t wb = (unit * kLanes + lane) * 16;  // the window's first byte from that boundary
    if (wb >= end) return;

    uint32_t acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    const char *tcol = reinterpret_cast<const char *>(tab) + 4 * (lane & (kCopies - 1));

    Input cur = input_of<kStriped>(p, stripe, 0, ulen);
    Raw raw = load_window(cur, a, wb);
#pragma unroll 1
    for (uint32_t j = 0; j < p.n_in; ++j) {
        Input nxt{0, 0};
        Raw nraw{};
        if (j + 1 < p.n_in) {
            nxt = input_of<kStriped>(p, stripe, j + 1, ulen);
            nraw = load_window(nxt, a, wb);
        }
        if (cur.len != 0) {
            uint32_t d[4];
            shift16(raw.c0, raw.c1, raw.sa, d);
            if (cur.len < ulen) {
                // a short cell: the window's bytes past the cell's end are zeros
                const uint64_t cend = a + cur.len;
                const uint32_t nv = cend > wb ? uint32_t(std::min<uint64_t>(cend - wb, 16)) : 0u;
#pragma unroll
                for (uint32_t g = 0; g < 4; ++g) {
                    const uint32_t keep = nv > 4 * g ? std::min(nv - 4 * g, 4u) : 0u;
                    d[g] &= keep >= 4 ? ~0u : (1u << (8 * keep)) - 1u;
                }
            }
            const char *tb = tcol + j * (hdfs_ec::kEntriesPerInput * kCopies * 4);
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t w = d[i >> 2] >> (8 * (i & 3u));
                const uint32_t lo = (w & 15u) << 7, hi = ((w >> 4) & 15u) << 7;  // entry * kCopies * 4
                acc[i] ^= *reinterpret_cast<const uint32_t *>(tb + lo) ^
                          *reinterpret_cast<const uint32_t *>(tb + 16 * kCopies * 4 + hi);
            }
        }
        cur = nxt;
        raw = nraw;
    }

    // acc[i] = (row 0, row 1, row 2, row 3) of byte position i: transpose 4 x 4
    uint32_t o[kMaxOut][4];
#pragma unroll
    for (uint32_t g = 0; g < 4; ++g) {
        const uint32_t a0 = acc[4 * g], a1 = acc[4 * g + 1], a2 = acc[4 * g + 2], a3 = acc[4 * g + 3];
        const uint32_t x0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u), x1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
        const uint32_t y0 = __builtin_amdgcn_perm(a3, a2, 0x05010400u), y1 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
        o[0][g] = __builtin_amdgcn_perm(y0, x0, 0x05040100u);
        o[1][g] = __builtin_amdgcn_perm(y0, x0, 0x07060302u);
        o[2][g] = __builtin_amdgcn_perm(y1, x1, 0x05040100u);
        o[3][g] = __builtin_amdgcn_perm(y1, x1, 0x07060302u);
    }

    const uint32_t lo_b = wb == 0 ? a : 0u;
    const uint32_t hi_b = end - wb < 16 ? uint32_t(end - wb) : 16u;
#pragma unroll
    for (uint32_t r = 0; r < kMaxOut; ++r) {
        if (r >= p.n_out) break;
        const uint64_t dst = p.out[r] + ooff - a + wb;  // the window's first byte in output r
        const uint32_t rel = uint32_t(dst) & 15u;       // (uniform: output r's phase against output 0)
        if (lo_b == 0 && hi_b == 16) {
            if (rel == 0) {
                *reinterpret_cast<GlobalU4>(dst) = U32x4{o[r][0], o[r][1], o[r][2], o[r][3]};
            } else if ((rel & 7u) == 0) {
                *reinterpret_cast<GlobalU2>(dst) = U32x2{o[r][0], o[r][1]};
                *reinterpret_cast<GlobalU2>(dst + 8) = U32x2{o[r][2], o[r][3]};
            } else if ((rel & 3u) == 0) {
#pragma unroll
                for (uint32_t g = 0; g < 4; ++g) *reinterpret_cast<GlobalU1>(dst + 4 * g) = o[r][g];
            } else if ((rel & 1u) == 0) {
#pragma unroll
                for (uint32_t h = 0; h < 8; ++h)
                    *reinterpret_cast<GlobalU16>(dst + 2 * h) = uint16_t(o[r][h >> 1] >> (16 * (h & 1u)));
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 16; ++b)
                    *reinterpret_cast<GlobalU8>(dst + b) = uint8_t(o[r][b >> 2] >> (8 * (b & 3u)));
            }
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b)
                if (b >= lo_b && b < hi_b) *reinterpret_cast<GlobalU8>(dst + b) = uint8_t(o[r][b >> 2] >> (8 * (b & 3u)));
        }
    }
}

// The copies of the nibble-table image (dword kCopies e + c = entry e).
__device__ __forceinline__ void build_tables(uint32_t *tab, const EcArgs &p) {
    const uint32_t e = threadIdx.x;
    if (e < p.n_in * hdfs_ec::kEntriesPerInput) {
        const uint32_t v = hdfs_ec::table_entry(p.coef, p.n_out, e);
#pragma unroll 4
        for (uint32_t c = 0; c < kCopies; ++c) tab[kCopies * e + ((c + e) & (kCopies - 1))] = v;
    }
    __syncthreads();
}

template <bool kStriped>
__global__ __launch_bounds__(kThreads) void hdfs_ec_kernel(const EcArgs p) {
    extern __shared__ uint32_t tab[];  // kLdsPerInput bytes per input
    build_tables(tab, p);
    const uint32_t lane = threadIdx.x & (kLanes - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    for (uint64_t g = blockIdx.x + uint64_t(gridDim.x) * wave; g < p.total; g += uint64_t(gridDim.x) * kWaves) {
        if (kStriped) {
            const uint64_t stripe = g / p.units_per_stripe;
            wave_unit<true>(p, tab, stripe, g - stripe * p.units_per_stripe, lane);
        } else {
            wave_unit<false>(p, tab, 0, g, lane);
        }
    }
}

// Wave units of a unit of len bytes whose output 0 is `a` bytes past a 16-byte boundary.
uint64_t wave_units(uint64_t len, uint32_t a) {
    const uint64_t windows = len ? (len >> 4) + (((len & 15u) + a + 15u) >> 4) : 0;
    return (windows + kLanes - 1) / kLanes;
}

int check_args(const char *who, const crc32c_ctx *ctx, const hdfs_ec_matrix *mx, EcArgs *p) {
    if (!ctx) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(-ENODEV, "no GPU");
        return fail(-EINVAL, "%s: ctx == NULL", who);
    }
    if (!mx) return fail(-EINVAL, "%s: mx == NULL", who);
    if (mx->n_in == 0 || mx->n_in > kMaxIn || mx->n_out == 0 || mx->n_out > kMaxOut)
        return fail(-EINVAL, "%s: a matrix of %u inputs and %u outputs (1 .. 16, 1 .. 4)", who, mx->n_in, mx->n_out);
    *p = EcArgs{};
    p->n_in = mx->n_in;
    p->n_out = mx->n_out;
    for (uint32_t r = 0; r < mx->n_out; ++r)
        for (uint32_t j = 0; j < mx->n_in; ++j) p->coef[r][j] = mx->coef[r][j];
    return 0;
}

bool overlap(uint64_t a, uint64_t alen, uint64_t b, uint64_t blen) { return a < b + blen && b < a + alen; }

// The outputs (olen bytes each) against each other.
int check_outputs(const char *who, const EcArgs &p, uint64_t olen) {
    for (uint32_t r = 0; r < p.n_out; ++r) {
        if (p.out[r] + olen < p.out[r]) return fail(-EINVAL, "%s: output %u: the address range wraps", who, r);
        for (uint32_t q = 0; q < r; ++q)
            if (overlap(p.out[r], olen, p.out[q], olen)) return fail(-EINVAL, "%s: output %u overlaps output %u", who, r, q);
    }
    return 0;
}

// Workgroups a CU holds at once: by their tables, at most kMaxWgPerCu.
uint32_t wg_per_cu(uint32_t n_in) { return std::min(kMaxWgPerCu, kLdsPerCu / (kLdsPerInput * n_in)); }

template <bool kStriped>
int launch(const crc32c_ctx *ctx, const EcArgs &p, hipStream_t s) {
    // (wave w of workgroup b takes units b + grid (w + kWaves i): a launch of few units still
    // spreads over every CU, with fewer busy waves per workgroup)
    const uint32_t grid = uint32_t(std::min<uint64_t>(p.total, uint64_t(std::max(ctx->num_cu, 1)) * wg_per_cu(p.n_in)));
    DeviceGuard guard(ctx->device);
    hipLaunchKernelGGL(hdfs_ec_kernel<kStriped>, dim3(grid, 1, 1), dim3(kThreads, 1, 1), p.n_in * kLdsPerInput, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

// Loads this file's code object onto the current device (crc32c_ctx_create,
// beside preload_aes_kernels).
hipError_t preload_ec_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&hdfs_ec_kernel<false>));
}

}  // namespace hdfs_crc

using namespace hdfs_crc;

extern "C" {

void crc32c_debug_ec_geometry(crc32c_debug_ec_geom *out) {
    if (!out) return;
    out->lane_bytes = 16;
    out->wave_bytes = 16 * kLanes;
    out->workgroup_bytes = 16 * kLanes * kWaves;
    out->waves_per_workgroup = kWaves;
    out->table_copies = kCopies;
    out->lds_bytes_per_input = kLdsPerInput;
    out->lds_bytes_per_cu = kLdsPerCu;
    out->max_workgroups_per_cu = kMaxWgPerCu;
}

int hdfs_ec_apply_dev(crc32c_ctx *ctx, const hdfs_ec_matrix *mx, const void *const *dev_in, void *const *dev_out,
                      uint64_t len, void *stream) {
    const char *who = "hdfs_ec_apply_dev";
    EcArgs p;
    if (int rc = check_args(who, ctx, mx, &p)) return rc;
    if (len == 0) return 0;
    if (!dev_in || !dev_out) return fail(-EINVAL, "%s: NULL pointer array with %llu bytes", who, (unsigned long long)len);
    if (len > (1ull << 62)) return fail(-EINVAL, "%s: more than 2^62 bytes", who);
    for (uint32_t r = 0; r < p.n_out; ++r) {
        p.out[r] = uint64_t(reinterpret_cast<uintptr_t>(dev_out[r]));
        if (!p.out[r]) return fail(-EINVAL, "%s: output %u: %llu bytes at NULL", who, r, (unsigned long long)len);
    }
    if (int rc = check_outputs(who, p, len)) return rc;
    for (uint32_t j = 0; j < p.n_in; ++j) {
        p.in[j] = uint64_t(reinterpret_cast<uintptr_t>(dev_in[j]));
        if (!p.in[j]) continue;  // a unit of zeros
        if (p.in[j] + len < p.in[j]) return fail(-EINVAL, "%s: input %u: the address range wraps", who, j);
        for (uint32_t r = 0; r < p.n_out; ++r)
            if (overlap(p.out[r], len, p.in[j], len)) return fail(-EINVAL, "%s: output %u overlaps input %u", who, r, j);
    }
    p.len = len;
    p.total = wave_units(len, uint32_t(p.out[0] & 15u));
    return launch<false>(ctx, p, static_cast<hipStream_t>(stream));
}

int hdfs_ec_encode_striped_dev(crc32c_ctx *ctx, const hdfs_ec_matrix *mx, const void *src, uint64_t len,
                               uint64_t cell, void *const *dev_parity, void *stream) {
    const char *who = "hdfs_ec_encode_striped_dev";
    EcArgs p;
    if (int rc = check_args(who, ctx, mx, &p)) return rc;
    if (cell == 0) return fail(-EINVAL, "%s: cell == 0", who);
    if (len == 0) return 0;
    if (!src || !dev_parity) return fail(-EINVAL, "%s: NULL pointer with %llu bytes", who, (unsigned long long)len);
    if (len > (1ull << 62)) return fail(-EINVAL, "%s: more than 2^62 bytes", who);
    if (cell > (1ull << 58)) return fail(-EINVAL, "%s: cells of more than 2^58 bytes", who);
    const uint64_t stripe = cell * p.n_in, nstripes = (len + stripe - 1) / stripe;
    // every parity block has the length of data block 0
    const uint64_t rest = len - (nstripes - 1) * stripe, plen = (nstripes - 1) * cell + std::min(rest, cell);
    p.in[0] = uint64_t(reinterpret_cast<uintptr_t>(src));
    if (p.in[0] + len < p.in[0]) return fail(-EINVAL, "%s: src: the address range wraps", who);
    for (uint32_t r = 0; r < p.n_out; ++r) {
        p.out[r] = uint64_t(reinterpret_cast<uintptr_t>(dev_parity[r]));
        if (!p.out[r]) return fail(-EINVAL, "%s: parity %u: %llu bytes at NULL", who, r, (unsigned long long)plen);
    }
    if (int rc = check_outputs(who, p, plen)) return rc;
    for (uint32_t r = 0; r < p.n_out; ++r)
        if (overlap(p.out[r], plen, p.in[0], len)) return fail(-EINVAL, "%s: parity %u overlaps src", who, r);
    p.len = len;
    p.cell = cell;
    // Every stripe has output 0's phase when the cell keeps it; otherwise a
    // stripe may spill into one more window than its length fills.
    const uint32_t a = (nstripes == 1 || (cell & 15u) == 0) ? uint32_t(p.out[0] & 15u) : 15u;
    p.units_per_stripe = wave_units(std::min(cell, len), a);
    p.total = nstripes * p.units_per_stripe;
    return launch<true>(ctx, p, static_cast<hipStream_t>(stream));
}

}  // extern "C"
