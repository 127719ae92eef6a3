"""Composite CRCs on the host (include/hdfs_crc32c.h section 6c):
crc32c_combine, crc32c_block_composite and crc32c_file_composite against the
CRC of the whole data -- zlib.crc32 for CRC32C_TYPE_CRC32, the oracle for
CRC32C, the reference's crc32c() too where its build exists -- and the
composite shape a packet batch gets at plan creation (host arithmetic,
through the debug hook; the plan objects themselves need the GPU and are in
tests/test_gpu_composite.py).  All results are bit-exact."""
from __future__ import annotations

import errno
import os
import zlib

import numpy as np
import pytest

import oracle

BE = 0x1     # CRC32C_BIG_ENDIAN
CRC32 = 0x2  # CRC32C_TYPE_CRC32


@pytest.fixture(scope="module")
def crc_of(orc):
    """crc_of(flags)(bytes) -> the oracle CRC of the polynomial in flags."""
    ref = oracle.Reference() if os.path.exists(oracle.REF_SO) else None

    def castagnoli(data) -> int:
        a = np.frombuffer(bytes(data), np.uint8)
        v = orc.crc32c(a)
        if ref is not None:
            assert ref.crc32c(a) == v
        return v

    def pick(flags):
        return (lambda d: zlib.crc32(bytes(d)) & 0xFFFFFFFF) if flags & CRC32 else castagnoli

    return pick


@pytest.fixture(scope="module")
def data():
    d = oracle.xorshift64_bytes(37 * 8192 + 64, 0xC0FFEE)
    d.setflags(write=False)
    return d


def chunk_sums(crc, buf, bpc, first=None):
    """The checksums of buf cut into a first chunk of `first` bytes (default bpc) and bpc-byte chunks;
    returns (sums, last_len)."""
    b = bytes(buf)
    first = bpc if first is None else first
    cuts = [0] + list(range(min(first, len(b)), len(b), bpc)) + [len(b)]
    cuts = sorted(set(cuts))
    sums = [crc(b[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]
    return np.array(sums, np.uint32), (cuts[-1] - cuts[-2] if len(cuts) > 1 else 0)


@pytest.mark.parametrize("flags", [0, CRC32])
def test_combine_against_the_oracle(hdfs, crc_of, data, flags):
    crc = crc_of(flags)
    for la in (0, 1, 3, 512, 700):
        for lb in (0, 1, 5, 512, 4096, 100000):
            a, b = bytes(data[:la]), bytes(data[la:la + lb])
            assert hdfs.combine(crc(a), crc(b), lb, flags) == crc(a + b), (la, lb)
    c = crc(bytes(data[:777]))
    for n in (0, 1, 512, 1 << 33):
        assert hdfs.combine(0, c, n, flags) == c
    assert hdfs.combine(c, 0, 0, flags) == c
    # associativity over three pieces
    p, q, r = bytes(data[:300]), bytes(data[300:1000]), bytes(data[1000:5001])
    left = hdfs.combine(hdfs.combine(crc(p), crc(q), len(q), flags), crc(r), len(r), flags)
    right = hdfs.combine(crc(p), hdfs.combine(crc(q), crc(r), len(r), flags), len(q) + len(r), flags)
    assert left == right == crc(p + q + r)


@pytest.mark.parametrize("flags", [0, CRC32])
@pytest.mark.parametrize("bpc", [1, 4, 512, 700, 4096, 8192])
def test_block_composite_against_the_whole_crc(hdfs, crc_of, data, flags, bpc):
    crc = crc_of(flags)
    for n in (1, 2, 3, 37):
        for last_len in sorted({1, max(bpc - 1, 1), bpc}):
            total = (n - 1) * bpc + last_len
            buf = data[11:11 + total]
            sums, last = chunk_sums(crc, buf, bpc)
            assert sums.size == n and last == last_len
            want = crc(buf)
            assert hdfs.block_composite(sums, bpc, last_len, flags) == want, (n, last_len)
            assert hdfs.block_composite(sums.byteswap(), bpc, last_len, flags | BE) == want, (n, last_len, "BE")
    # a short first chunk: its length never enters
    for first in sorted({1, max(bpc // 2, 1)}):
        buf = data[5:5 + first + 4 * bpc + 1]
        sums, last = chunk_sums(crc, buf, bpc, first=first)
        assert sums.size == 6 and last == 1
        assert hdfs.block_composite(sums, bpc, last, flags) == crc(buf)


@pytest.mark.parametrize("flags", [0, CRC32])
def test_long_block_takes_the_table_path(hdfs, crc_of, data, flags):
    """More checksums than the table threshold, against the oracle."""
    crc = crc_of(flags)
    buf = data[:199 * 512 + 77]
    sums, last = chunk_sums(crc, buf, 512)
    assert sums.size == 200
    assert hdfs.block_composite(sums, 512, last, flags) == crc(buf)


@pytest.mark.parametrize("flags", [0, CRC32])
def test_bpc_independence(hdfs, crc_of, data, flags):
    crc = crc_of(flags)
    buf = data[:200000]
    want = crc(buf)
    got = []
    for bpc in (512, 1024, 4096, 700):
        sums, last = chunk_sums(crc, buf, bpc)
        got.append(hdfs.block_composite(sums, bpc, last, flags))
    assert got == [want] * 4


@pytest.mark.parametrize("flags", [0, CRC32])
def test_file_composite(hdfs, crc_of, data, flags):
    crc = crc_of(flags)
    lens = [65536, 0, 100000, 1, 30000]
    cuts = np.concatenate([[0], np.cumsum(lens)])
    blocks = [bytes(data[cuts[i]:cuts[i + 1]]) for i in range(len(lens))]
    crcs = [crc(b) for b in blocks]
    assert crcs[1] == 0
    assert hdfs.file_composite(crcs, lens, flags) == crc(b"".join(blocks))
    assert hdfs.file_composite([], [], flags) == 0
    # blocks under one bpc: the file's value is block_composite over the concatenated checksum array
    lens2 = [4096 * 3, 4096 * 5, 4096 * 2 + 100]
    cuts2 = np.concatenate([[0], np.cumsum(lens2)])
    per_block, all_sums = [], []
    for i in range(3):
        sums, last = chunk_sums(crc, data[cuts2[i]:cuts2[i + 1]], 4096)
        per_block.append(hdfs.block_composite(sums, 4096, last, flags))
        all_sums.append(sums)
    whole = hdfs.block_composite(np.concatenate(all_sums), 4096, 100, flags)
    assert hdfs.file_composite(per_block, lens2, flags) == whole == crc(data[:cuts2[-1]])


def test_argument_errors(hdfs):
    sums = np.arange(4, dtype=np.uint32)
    refused = [
        lambda: hdfs.block_composite(sums, 0, 1),
        lambda: hdfs.block_composite(sums, 512, 0),
        lambda: hdfs.block_composite(sums, 512, 513),
        lambda: hdfs.block_composite(sums, 512, 512, flags=0x4),
        lambda: hdfs.block_composite(np.zeros(0, np.uint32), 0, 1),
        lambda: hdfs.file_composite([1], [1], flags=BE),
        lambda: hdfs.file_composite([1], [1], flags=0x8),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == -errno.EINVAL, k
    assert hdfs.block_composite(np.zeros(0, np.uint32), 512, 0) == 0  # n == 0: last_len is not looked at
    assert hdfs.lib().crc32c_block_composite(None, 0, 512, 512, 0, None) == -errno.EINVAL
    assert hdfs.lib().crc32c_block_composite(None, 3, 512, 512, 0, sums.ctypes.data) == -errno.EINVAL
    assert hdfs.lib().crc32c_file_composite(None, None, 2, 0, sums.ctypes.data) == -errno.EINVAL
    assert hdfs.COMPOSITE_LIST_MAX_BLOCKS * 16 + 160 <= 4096


def _pk(hdfs, rows):
    return np.array(rows, dtype=hdfs.PACKET_DTYPE)


def test_composite_shape_of_packet_batches(hdfs):
    """What crc32c_plan_create records (rows: payload_off, out_idx, len, bpc)."""
    shape = hdfs.debug_packets_composite_shape
    assert shape(oracle.uniform_packets(4, 65536, 512)) == (512, 512)  # uniform
    assert shape(_pk(hdfs, [(0, 0, 65536, 512), (65536, 128, 1000, 512), (66536, 130, 0, 512)])) == (512, 488)
    assert shape(_pk(hdfs, [(0, 0, 300, 512), (300, 1, 65536, 512), (65836, 129, 5, 512)])) == (512, 5)  # unaligned first
    assert shape(_pk(hdfs, [(0, 0, 77, 700)])) == (700, 77)  # one short chunk: first and last
    # the same packets in another order
    assert shape(_pk(hdfs, [(65536, 128, 1000, 512), (0, 0, 65536, 512)])) == (512, 488)
    assert shape(oracle.mixed_packets(6)) is None                                        # mixed bpc
    assert shape(_pk(hdfs, [(0, 0, 1024, 512), (1024, 2, 100, 512), (1124, 3, 1024, 512)])) is None  # short middle
    assert shape(_pk(hdfs, [(0, 0, 300, 512), (300, 1, 300, 512), (600, 2, 512, 512)])) is None      # second short
    assert shape(_pk(hdfs, [(0, 0, 1024, 512), (1024, 3, 1024, 512)])) is None            # out_idx gap
    assert shape(_pk(hdfs, [(0, 1, 1024, 512)])) is None                                  # does not start at 0
    assert shape(_pk(hdfs, [(0, 0, 1024, 512), (1024, 1, 1024, 512)])) is None            # overlap
    assert shape(_pk(hdfs, [(0, 0, 0, 512)])) is None                                     # nothing to combine


def test_geometry_hook(hdfs):
    g = hdfs.debug_composite_geometry()
    assert g["lanes"] == 64 and g["run"] >= 1 and g["waves_per_workgroup"] >= 1
    assert g["split_above"] == g["run"] * g["lanes"] + 1
