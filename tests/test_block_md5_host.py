"""Host side of the block MD5-of-CRCs feature (include/hdfs_crc32c.h section
6b): crc32c_file_md5 (the MD5-of-MD5-of-CRC file checksum's digest),
crc32c_md5_nblocks, and the argument errors of the device calls that are
decided before any device is touched.  No GPU."""
from __future__ import annotations

import ctypes
import errno
import hashlib

import numpy as np
import pytest


def _digests(n):
    rng = np.random.default_rng(1000 + n)
    return rng.integers(0, 256, 16 * n, dtype=np.uint8)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5])
def test_file_md5_matches_hashlib(hdfs, n):
    """0 digests = the empty message; 4 digests are exactly one 64-byte MD5
    block (the padding forms a block of its own); 3 and 5 sit either side."""
    d = _digests(n)
    want = hashlib.md5(d.tobytes()).digest()
    assert hdfs.file_md5(d) == want
    assert hdfs.file_md5(d.tobytes()) == want


def test_file_md5_rejects_partial_digest(hdfs):
    with pytest.raises(ValueError):
        hdfs.file_md5(bytes(17))


@pytest.mark.parametrize("nsums,cpb,want", [(0, 8, 0), (1, 8, 1), (8, 8, 1), (9, 8, 2)])
def test_md5_nblocks(hdfs, nsums, cpb, want):
    assert hdfs.md5_nblocks(nsums, cpb) == want


def test_md5_nblocks_large_and_zero_divisor(hdfs):
    assert hdfs.md5_nblocks((1 << 40) + 1, 8192) == (1 << 27) + 1
    assert hdfs.md5_nblocks(5, 0) == 0


def _last_error(hdfs) -> str:
    return hdfs.lib().crc32c_last_error().decode()


def test_null_context_is_einval(hdfs):
    """ctx == NULL: -EINVAL from both context calls whatever else is passed
    (the addresses below are never dereferenced: nothing is launched)."""
    L = hdfs.lib()
    vp = ctypes.c_void_p
    rc = L.crc32c_md5_blocks(None, vp(0x1000), 16, 8, 0, vp(0x2000), None)
    assert rc == -errno.EINVAL and "ctx" in _last_error(hdfs)
    rc = L.crc32c_md5_blocks(None, None, 0, 8, 0, vp(0x2000), None)  # (even with nothing to do)
    assert rc == -errno.EINVAL
    ptrs = (ctypes.c_void_p * 1)(0x1000)
    counts = (ctypes.c_uint32 * 1)(4)
    rc = L.crc32c_md5_block_list(None, ptrs, counts, 1, 0, vp(0x2000), None)
    assert rc == -errno.EINVAL and "ctx" in _last_error(hdfs)


def test_null_plan_is_einval(hdfs):
    L = hdfs.lib()
    pays = (ctypes.c_void_p * 1)(0x1000)
    outs = (ctypes.c_void_p * 1)(0x3000)
    rc = L.crc32c_plan_exec_blocks_md5(None, pays, outs, 1, ctypes.c_void_p(0x2000), None)
    assert rc == -errno.EINVAL and "plan" in _last_error(hdfs)


def test_python_wrappers_raise_on_null_context(hdfs):
    """Context.md5_blocks / md5_block_list on a closed context (handle None = NULL)."""
    ctx = hdfs.Context.__new__(hdfs.Context)
    ctx.handle = None
    ctx.device = 0
    with pytest.raises(hdfs.Crc32cError) as e:
        ctx.md5_blocks(0x1000, 16, 8, 0x2000)
    assert e.value.rc == -errno.EINVAL
    with pytest.raises(hdfs.Crc32cError) as e:
        ctx.md5_block_list([0x1000], [4], 0x2000)
    assert e.value.rc == -errno.EINVAL
    with pytest.raises(ValueError):
        ctx.md5_block_list([0x1000], [4, 5], 0x2000)
