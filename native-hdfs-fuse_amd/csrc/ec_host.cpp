// ec_host.cpp -- erasure coding on the host (include/hdfs_crc32c.h section
// 8): the Cauchy encode matrix, the decode matrix of an erasure pattern, the
// layout of a striped block group, the packets of a data block over the
// file-order buffer, and the portable nibble-table multiply (the CPU path and
// the GPU tests' oracle).  No allocation, no state.
#include <cerrno>
#include <cstring>

#include "ec_gf256.h"
#include "errors.h"
#include "hdfs_crc32c.h"

namespace {

using hdfs_crc::fail;
using hdfs_ec::kMaxIn;
using hdfs_ec::kMaxOut;

int check_scheme(const char *who, int codec, uint32_t k, uint32_t m) {
    if (codec != HDFS_EC_RS && codec != HDFS_EC_XOR) return fail(-EINVAL, "%s: codec %d (HDFS_EC_RS or HDFS_EC_XOR)", who, codec);
    if (k == 0 || k > kMaxIn) return fail(-EINVAL, "%s: %u data units (1 .. 16)", who, k);
    if (m == 0 || m > kMaxOut) return fail(-EINVAL, "%s: %u parity units (1 .. 4)", who, m);
    if (codec == HDFS_EC_XOR && m != 1) return fail(-EINVAL, "%s: the XOR codec has one parity unit (%u given)", who, m);
    return 0;
}

// Row `unit` of the generator [I_k ; P].
void generator_row(int codec, uint32_t k, uint32_t unit, uint8_t row[kMaxIn]) {
    for (uint32_t j = 0; j < k; ++j)
        row[j] = unit < k ? uint8_t(unit == j) : codec == HDFS_EC_XOR ? uint8_t(1) : uint8_t(hdfs_ec::cauchy(k, unit - k, j));
}

int check_matrix(const char *who, const hdfs_ec_matrix *mx) {
    if (!mx) return fail(-EINVAL, "%s: mx == NULL", who);
    if (mx->n_in == 0 || mx->n_in > kMaxIn || mx->n_out == 0 || mx->n_out > kMaxOut)
        return fail(-EINVAL, "%s: a matrix of %u inputs and %u outputs (1 .. 16, 1 .. 4)", who, mx->n_in, mx->n_out);
    return 0;
}

}  // namespace

extern "C" {

uint8_t hdfs_gf256_mul(uint8_t a, uint8_t b) { return uint8_t(hdfs_ec::mul(a, b)); }
uint8_t hdfs_gf256_inv(uint8_t a) { return uint8_t(hdfs_ec::inv(a)); }

int hdfs_ec_encode_matrix(int codec, uint32_t k, uint32_t m, hdfs_ec_matrix *out) {
    if (!out) return fail(-EINVAL, "hdfs_ec_encode_matrix: out == NULL");
    if (int rc = check_scheme("hdfs_ec_encode_matrix", codec, k, m)) return rc;
    std::memset(out, 0, sizeof *out);
    out->n_in = k;
    out->n_out = m;
    for (uint32_t r = 0; r < m; ++r) generator_row(codec, k, k + r, out->coef[r]);
    return 0;
}

int hdfs_ec_decode_matrix(int codec, uint32_t k, uint32_t m, const uint32_t *valid, const uint32_t *erased,
                          uint32_t n_erased, hdfs_ec_matrix *out) {
    const char *who = "hdfs_ec_decode_matrix";
    if (!out || !valid || !erased) return fail(-EINVAL, "%s: NULL argument", who);
    if (int rc = check_scheme(who, codec, k, m)) return rc;
    if (n_erased == 0 || n_erased > kMaxOut) return fail(-EINVAL, "%s: %u erased units (1 .. 4)", who, n_erased);
    uint32_t seen = 0;  // (k + m <= 20 units)
    for (uint32_t i = 0; i < k; ++i) {
        if (valid[i] >= k + m) return fail(-EINVAL, "%s: valid[%u] = %u of %u units", who, i, valid[i], k + m);
        if (seen >> valid[i] & 1u) return fail(-EINVAL, "%s: unit %u is listed twice as valid", who, valid[i]);
        seen |= 1u << valid[i];
    }
    uint32_t gone = 0;
    for (uint32_t i = 0; i < n_erased; ++i) {
        if (erased[i] >= k + m) return fail(-EINVAL, "%s: erased[%u] = %u of %u units", who, i, erased[i], k + m);
        if (gone >> erased[i] & 1u) return fail(-EINVAL, "%s: unit %u is listed twice as erased", who, erased[i]);
        if (seen >> erased[i] & 1u) return fail(-EINVAL, "%s: unit %u is both valid and erased", who, erased[i]);
        gone |= 1u << erased[i];
    }
    uint8_t s[kMaxIn][kMaxIn], si[kMaxIn][kMaxIn];
    for (uint32_t i = 0; i < k; ++i) generator_row(codec, k, valid[i], s[i]);
    if (!hdfs_ec::invert(s, si, k)) return fail(-EINVAL, "%s: the surviving rows are singular", who);
    std::memset(out, 0, sizeof *out);
    out->n_in = k;
    out->n_out = n_erased;
    for (uint32_t r = 0; r < n_erased; ++r) {
        uint8_t g[kMaxIn];
        generator_row(codec, k, erased[r], g);
        // (row e of S^-1 for a data unit: g is then row e of the identity)
        for (uint32_t i = 0; i < k; ++i) {
            uint32_t v = 0;
            for (uint32_t j = 0; j < k; ++j) v ^= hdfs_ec::mul(g[j], si[j][i]);
            out->coef[r][i] = uint8_t(v);
        }
    }
    return 0;
}

int hdfs_ec_group_layout(uint64_t len, uint32_t k, uint32_t m, uint64_t cell, uint64_t *block_len) {
    const char *who = "hdfs_ec_group_layout";
    if (!block_len) return fail(-EINVAL, "%s: block_len == NULL", who);
    if (int rc = check_scheme(who, HDFS_EC_RS, k, m)) return rc;
    if (cell == 0) return fail(-EINVAL, "%s: cell == 0", who);
    if (cell > UINT64_MAX / k) return fail(-EINVAL, "%s: a stripe of %u cells of %llu bytes exceeds 2^64", who, k, (unsigned long long)cell);
    const uint64_t stripe = cell * k, full = len / stripe, rest = len % stripe;
    for (uint32_t b = 0; b < k; ++b) {
        const uint64_t before = uint64_t(b) * cell;
        block_len[b] = full * cell + (rest <= before ? 0 : rest - before < cell ? rest - before : cell);
    }
    for (uint32_t r = 0; r < m; ++r) block_len[k + r] = block_len[0];
    return 0;
}

int64_t hdfs_ec_block_packets(uint64_t len, uint32_t k, uint64_t cell, uint32_t block, uint32_t packetsize,
                              uint32_t bpc, uint64_t out_idx0, crc32c_packet *pkts, size_t cap) {
    const char *who = "hdfs_ec_block_packets";
    if (k == 0 || k > kMaxIn) return fail(-EINVAL, "%s: %u data units (1 .. 16)", who, k);
    if (block >= k) return fail(-EINVAL, "%s: data block %u of %u", who, block, k);
    if (cell == 0 || packetsize == 0 || bpc == 0) return fail(-EINVAL, "%s: cell, packetsize and bpc must be positive", who);
    if (cell % packetsize != 0) return fail(-EINVAL, "%s: cell %llu is not a multiple of packetsize %u", who, (unsigned long long)cell, packetsize);
    if (packetsize % bpc != 0) return fail(-EINVAL, "%s: packetsize %u is not a multiple of bpc %u", who, packetsize, bpc);
    if (cell > UINT64_MAX / k) return fail(-EINVAL, "%s: a stripe of %u cells of %llu bytes exceeds 2^64", who, k, (unsigned long long)cell);
    const uint64_t stripe = cell * k, full = len / stripe, rest = len % stripe, before = uint64_t(block) * cell;
    const uint64_t blen = full * cell + (rest <= before ? 0 : rest - before < cell ? rest - before : cell);
    const uint64_t n = (blen + packetsize - 1) / packetsize;
    if (n > uint64_t(INT64_MAX)) return fail(-EINVAL, "%s: too many packets", who);
    if (!pkts) return int64_t(n);
    if (cap < n) return fail(-EINVAL, "%s: room for %zu of %llu packets", who, cap, (unsigned long long)n);
    const uint64_t sums_per_packet = packetsize / bpc;
    for (uint64_t p = 0; p < n; ++p) {
        // a packet never straddles a cell (cell % packetsize == 0)
        const uint64_t off = p * packetsize;
        pkts[p].payload_off = (off / cell) * stripe + before + off % cell;
        pkts[p].out_idx = out_idx0 + p * sums_per_packet;
        pkts[p].len = uint32_t(blen - off < packetsize ? blen - off : packetsize);
        pkts[p].bpc = bpc;
    }
    return int64_t(n);
}

int hdfs_ec_apply(const hdfs_ec_matrix *mx, const void *const *in, void *const *out, size_t len) {
    const char *who = "hdfs_ec_apply";
    if (int rc = check_matrix(who, mx)) return rc;
    if (len == 0) return 0;
    if (!in || !out) return fail(-EINVAL, "%s: NULL pointer array with %zu bytes", who, len);
    for (uint32_t r = 0; r < mx->n_out; ++r) {
        if (!out[r]) return fail(-EINVAL, "%s: out[%u] == NULL with %zu bytes", who, r, len);
        const uintptr_t o = uintptr_t(out[r]);
        for (uint32_t j = 0; j < mx->n_in; ++j)
            if (in[j] && uintptr_t(in[j]) < o + len && o < uintptr_t(in[j]) + len)
                return fail(-EINVAL, "%s: out[%u] overlaps in[%u]", who, r, j);
        for (uint32_t q = 0; q < r; ++q)
            if (uintptr_t(out[q]) < o + len && o < uintptr_t(out[q]) + len)
                return fail(-EINVAL, "%s: out[%u] overlaps out[%u]", who, r, q);
    }
    uint32_t tab[kMaxIn * hdfs_ec::kEntriesPerInput];
    for (uint32_t e = 0; e < mx->n_in * hdfs_ec::kEntriesPerInput; ++e) tab[e] = hdfs_ec::table_entry(mx->coef, mx->n_out, e);
    constexpr size_t kStep = 256;
    uint32_t acc[kStep];
    for (size_t t0 = 0; t0 < len; t0 += kStep) {
        const size_t n = len - t0 < kStep ? len - t0 : kStep;
        std::memset(acc, 0, sizeof acc);
        for (uint32_t j = 0; j < mx->n_in; ++j) {
            if (!in[j]) continue;
            const uint8_t *p = static_cast<const uint8_t *>(in[j]) + t0;
            const uint32_t *lo = tab + 32 * j, *hi = lo + 16;
            for (size_t t = 0; t < n; ++t) acc[t] ^= lo[p[t] & 15u] ^ hi[p[t] >> 4];
        }
        for (uint32_t r = 0; r < mx->n_out; ++r) {
            uint8_t *q = static_cast<uint8_t *>(out[r]) + t0;
            for (size_t t = 0; t < n; ++t) q[t] = uint8_t(acc[t] >> (8 * r));
        }
    }
    return 0;
}

}  // extern "C"
