// aes_ctr_host.cpp -- AES/CTR/NoPadding on the host (include/hdfs_crc32c.h
// section 7): key expansion, Hadoop's calculateIV, the portable T-table
// keystream (the CPU path and the GPU tests' oracle) and the stream layout of
// a batch of packets on an encrypted transfer.  No allocation, no state.
#include <cerrno>
#include <cstring>

#include "aes_ctr.h"
#include "errors.h"
#include "hdfs_crc32c.h"

namespace {

using hdfs_crc::fail;

constexpr hdfs_aes::Tables kT;

inline uint32_t load_be32(const uint8_t *p) {
    return uint32_t(p[0]) << 24 | uint32_t(p[1]) << 16 | uint32_t(p[2]) << 8 | p[3];
}

// AES_K of the counter block (hi, lo) as 16 keystream bytes.
void keystream_block(const hdfs_aes_ctr *c, uint64_t hi, uint64_t lo, uint8_t out[16]) {
    const uint32_t *rk = c->rk;
    uint32_t s0 = uint32_t(hi >> 32) ^ rk[0], s1 = uint32_t(hi) ^ rk[1], s2 = uint32_t(lo >> 32) ^ rk[2],
             s3 = uint32_t(lo) ^ rk[3];
    const auto &te = kT.te;
    for (uint32_t r = 1; r < c->rounds; ++r) {
        rk += 4;
        const uint32_t t0 = te[0][s0 >> 24] ^ te[1][(s1 >> 16) & 255] ^ te[2][(s2 >> 8) & 255] ^ te[3][s3 & 255] ^ rk[0];
        const uint32_t t1 = te[0][s1 >> 24] ^ te[1][(s2 >> 16) & 255] ^ te[2][(s3 >> 8) & 255] ^ te[3][s0 & 255] ^ rk[1];
        const uint32_t t2 = te[0][s2 >> 24] ^ te[1][(s3 >> 16) & 255] ^ te[2][(s0 >> 8) & 255] ^ te[3][s1 & 255] ^ rk[2];
        const uint32_t t3 = te[0][s3 >> 24] ^ te[1][(s0 >> 16) & 255] ^ te[2][(s1 >> 8) & 255] ^ te[3][s2 & 255] ^ rk[3];
        s0 = t0, s1 = t1, s2 = t2, s3 = t3;
    }
    rk += 4;
    const uint8_t *sb = kT.s;
    const uint32_t t[4] = {
        (uint32_t(sb[s0 >> 24]) << 24 | uint32_t(sb[(s1 >> 16) & 255]) << 16 | uint32_t(sb[(s2 >> 8) & 255]) << 8 | sb[s3 & 255]) ^ rk[0],
        (uint32_t(sb[s1 >> 24]) << 24 | uint32_t(sb[(s2 >> 16) & 255]) << 16 | uint32_t(sb[(s3 >> 8) & 255]) << 8 | sb[s0 & 255]) ^ rk[1],
        (uint32_t(sb[s2 >> 24]) << 24 | uint32_t(sb[(s3 >> 16) & 255]) << 16 | uint32_t(sb[(s0 >> 8) & 255]) << 8 | sb[s1 & 255]) ^ rk[2],
        (uint32_t(sb[s3 >> 24]) << 24 | uint32_t(sb[(s0 >> 16) & 255]) << 16 | uint32_t(sb[(s1 >> 8) & 255]) << 8 | sb[s2 & 255]) ^ rk[3]};
    for (int i = 0; i < 4; ++i) {
        out[4 * i] = uint8_t(t[i] >> 24);
        out[4 * i + 1] = uint8_t(t[i] >> 16);
        out[4 * i + 2] = uint8_t(t[i] >> 8);
        out[4 * i + 3] = uint8_t(t[i]);
    }
}

}  // namespace

extern "C" {

int hdfs_aes_ctr_init(hdfs_aes_ctr *c, const uint8_t *key, uint32_t key_bits, const uint8_t iv[16]) {
    if (!c || !key || !iv) return fail(-EINVAL, "hdfs_aes_ctr_init: NULL argument");
    const uint32_t rounds = hdfs_aes::expand_key(kT.s, key, key_bits, c->rk);
    if (!rounds) {
        std::memset(c, 0, sizeof *c);
        return fail(-EINVAL, "hdfs_aes_ctr_init: key of %u bits (128, 192 or 256)", key_bits);
    }
    std::memcpy(c->iv, iv, 16);
    c->rounds = rounds;
    c->reserved[0] = c->reserved[1] = c->reserved[2] = 0;
    return 0;
}

void hdfs_aes_ctr_counter(const uint8_t iv[16], uint64_t block_index, uint8_t out[16]) {
    uint64_t hi, lo;
    hdfs_aes::ctr_add(hdfs_aes::load_be64(iv), hdfs_aes::load_be64(iv + 8), block_index, &hi, &lo);
    hdfs_aes::store_be64(out, hi);
    hdfs_aes::store_be64(out + 8, lo);
}

int hdfs_aes_ctr_xor(const hdfs_aes_ctr *c, uint64_t stream_off, const void *in, void *out, size_t len) {
    if (!c) return fail(-EINVAL, "hdfs_aes_ctr_xor: c == NULL");
    if (c->rounds != 10 && c->rounds != 12 && c->rounds != 14)
        return fail(-EINVAL, "hdfs_aes_ctr_xor: %u rounds (hdfs_aes_ctr_init sets 10, 12 or 14)", c->rounds);
    if (len == 0) return 0;
    if (!in || !out) return fail(-EINVAL, "hdfs_aes_ctr_xor: NULL buffer with %zu bytes", len);
    if (stream_off + uint64_t(len) < stream_off && stream_off + uint64_t(len) != 0)
        return fail(-EINVAL, "hdfs_aes_ctr_xor: stream_off + len exceeds 2^64");
    const uint8_t *src = static_cast<const uint8_t *>(in);
    uint8_t *dst = static_cast<uint8_t *>(out);
    const uint64_t ivhi = hdfs_aes::load_be64(c->iv), ivlo = hdfs_aes::load_be64(c->iv + 8);
    uint64_t block = stream_off >> 4;
    uint32_t phase = uint32_t(stream_off & 15);
    uint8_t ks[16];
    while (len) {
        uint64_t hi, lo;
        hdfs_aes::ctr_add(ivhi, ivlo, block, &hi, &lo);
        keystream_block(c, hi, lo, ks);
        const size_t n = len < 16 - phase ? len : 16 - phase;
        if (n == 16) {
            uint64_t a, b, ka, kb;  // (memcpy: any alignment, in place allowed)
            std::memcpy(&a, src, 8);
            std::memcpy(&b, src + 8, 8);
            std::memcpy(&ka, ks, 8);
            std::memcpy(&kb, ks + 8, 8);
            a ^= ka;
            b ^= kb;
            std::memcpy(dst, &a, 8);
            std::memcpy(dst + 8, &b, 8);
        } else {
            for (size_t i = 0; i < n; ++i) dst[i] = src[i] ^ ks[phase + i];
        }
        src += n;
        dst += n;
        len -= n;
        phase = 0;
        ++block;
    }
    return 0;
}

int64_t hdfs_aes_wire_segments(const crc32c_packet *pkts, size_t npkts, const uint64_t *prefix_off,
                               uint64_t stream_base, const void *src_base, void *dst_base,
                               hdfs_aes_segment *data_segs, uint64_t *prefix_stream_off, size_t cap) {
    if (npkts == 0) return 0;
    if (!pkts || !prefix_off) return fail(-EINVAL, "hdfs_aes_wire_segments: pkts/prefix_off == NULL");
    if (cap < npkts) return fail(-EINVAL, "hdfs_aes_wire_segments: room for %zu of %zu packets", cap, npkts);
    if (!data_segs || !prefix_stream_off) return fail(-EINVAL, "hdfs_aes_wire_segments: NULL output");
    uint64_t data_before = 0;
    for (size_t i = 0; i < npkts; ++i) {
        if (prefix_off[i + 1] < prefix_off[i]) return fail(-EINVAL, "hdfs_aes_wire_segments: prefix_off decreases at %zu", i);
        // prefix 0, data 0, prefix 1, data 1, ...: packet i's prefix follows
        // i prefixes and the data of packets 0 .. i - 1
        const uint64_t pre = stream_base + prefix_off[i] + data_before;
        const uint64_t data = stream_base + prefix_off[i + 1] + data_before;
        if (pre < stream_base || data < pre || data + pkts[i].len < data)
            return fail(-EINVAL, "hdfs_aes_wire_segments: the stream exceeds 2^64 at packet %zu", i);
        prefix_stream_off[i] = pre;
        data_segs[i].src = reinterpret_cast<const void *>(uintptr_t(src_base) + uintptr_t(pkts[i].payload_off));
        data_segs[i].dst = reinterpret_cast<void *>(uintptr_t(dst_base) + uintptr_t(pkts[i].payload_off));
        data_segs[i].stream_off = data;
        data_segs[i].len = pkts[i].len;
        data_before += pkts[i].len;
    }
    return int64_t(npkts);
}

}  // extern "C"
