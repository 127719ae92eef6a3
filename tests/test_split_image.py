"""The split S4 image (16 columns per byte table) and its lookup addresses.

CPU only.  The split image is derived from the full S4 image
(``crc32c_debug_lds_image_s4``, pinned elsewhere); here its content is checked
against the full image's, and a mirror of the kernel's address arithmetic
(``s4<kImgSplit>`` in csrc/crc32c_device.h) is checked lane by lane: every
lookup of a step reads the right table's entry for the right byte, the 32
lookups of one instruction in a half-wave fall on 32 different LDS banks
whatever the data, and the step equals KernelModelS4's S."""
from __future__ import annotations

import numpy as np
import pytest

from kernel_model import KernelModelS4

FULL_NIB_OFF, FULL_SHIFT_OFF = 131072, 147456
NIB_OFF, SHIFT_OFF = 65536, 81920
SPLIT_BYTES = SHIFT_OFF + 15 * 512


@pytest.fixture(scope="module", params=[0, 1], ids=["crc32c", "crc32"])
def images(hdfs, request):
    flags = hdfs.CRC32C_TYPE_CRC32 if request.param else 0
    return hdfs.debug_lds_image_s4(flags), hdfs.debug_lds_image_s4_split(flags)


def _full_t(full: np.ndarray, m: int) -> np.ndarray:
    """T_m[b] from column 0 of the full image."""
    b = np.arange(256)
    return full.view("<u4")[((m >> 1) * 65536 + b * 256 + (m & 1) * 128) // 4]


def test_sizes_and_staging_chunks(images):
    full, split = images
    assert split.size == SPLIT_BYTES == 89600
    assert (split.size + 1023) // 1024 == 88
    assert SHIFT_OFF % 1024 == 0 and SHIFT_OFF // 1024 == 80  # (skip_z: the Z section starts on a chunk)
    assert full.size == FULL_SHIFT_OFF + 15 * 512


def test_every_t_entry_is_the_full_images(images):
    full, split = images
    w = split.view("<u4")
    b = np.arange(256)[:, None]
    c = np.arange(16)[None, :]
    for m in range(4):
        got = w[(b * 256 + m * 64 + 4 * c) // 4]
        assert np.array_equal(got, np.broadcast_to(_full_t(full, m)[:, None], got.shape)), m


def test_nq_and_z_sections_are_the_full_images(images):
    full, split = images
    assert np.array_equal(split[NIB_OFF:SHIFT_OFF], full[FULL_NIB_OFF:FULL_SHIFT_OFF])
    assert np.array_equal(split[SHIFT_OFF:], full[FULL_SHIFT_OFF:])


# ---- the kernel's address arithmetic, mirrored -----------------------------
# Per lane column q: col4 = 4 q (q < 16: T0's columns, q >= 16: T1's, at +64)
# and col4 ^ 64 (the other table of the pair); the T2 / T3 pair sits 128 bytes
# on.  Lookup A reads base col4 with byte 3 of v (q < 16) or byte 2 (q >= 16),
# lookup B base col4 ^ 64 with the bytes swapped, lookups C / D the same at
# +128 with bytes 1 / 0.  Each entry: (address, table, byte index).
def lookups(v: np.ndarray, q: np.ndarray):
    v = v.astype(np.int64)
    q = q.astype(np.int64)
    col4 = 4 * q
    colx = col4 ^ 64
    lo = q < 16

    def byte(j):
        return (v >> (8 * j)) & 0xFF

    ja, jb = np.where(lo, 3, 2), np.where(lo, 2, 3)
    jc, jd = np.where(lo, 1, 0), np.where(lo, 0, 1)
    out = []
    for base, j, imm in ((col4, ja, 0), (colx, jb, 0), (col4, jc, 128), (colx, jd, 128)):
        out.append(((byte(j) << 8) | base) + imm)
    tables = (np.where(lo, 0, 1), np.where(lo, 1, 0), np.where(lo, 2, 3), np.where(lo, 3, 2))
    return list(zip(out, tables, (ja, jb, jc, jd)))


def _data_sets():
    rng = np.random.default_rng(20240611)
    q = np.arange(32)
    sets = [("random", rng.integers(0, 2 ** 32, size=(64, 32), dtype=np.uint64).astype(np.uint32))]
    eq = np.repeat(rng.integers(0, 256, size=(32, 1), dtype=np.uint64), 32, axis=1)
    sets.append(("all-equal bytes", (eq * 0x01010101).astype(np.uint32)))
    # all-distinct bytes: lane q's four bytes are 4 q .. 4 q + 3 (rotated per row)
    rot = np.arange(8)[:, None]
    b0 = (4 * q[None, :] + rot) & 0xFF
    dist = b0 | (((b0 + 1) & 0xFF) << 8) | (((b0 + 2) & 0xFF) << 16) | (((b0 + 3) & 0xFF) << 24)
    sets.append(("all-distinct bytes", dist.astype(np.uint32)))
    return sets, q


def test_each_lookup_reads_the_right_entry(images):
    full, split = images
    w = split.view("<u4")
    sets, q = _data_sets()
    t_full = [_full_t(full, m) for m in range(4)]
    for name, v in sets:
        qq = np.broadcast_to(q[None, :], v.shape)
        seen = []
        for addr, table, j in lookups(v, qq):
            assert addr.min() >= 0 and addr.max() < NIB_OFF and not (addr & 3).any(), name
            b = (v.astype(np.int64) >> (8 * j)) & 0xFF
            for m in range(4):
                sel = table == m
                assert np.array_equal(w[addr[sel] // 4], t_full[m][b[sel]]), (name, m)
            seen.append((table, j))
        # the four lookups of a lane cover T3[b0], T2[b1], T1[b2], T0[b3] exactly once
        pairs = np.stack([t * 4 + j for t, j in seen])
        assert np.array_equal(np.sort(pairs, axis=0),
                              np.broadcast_to(np.array([3, 6, 9, 12])[:, None, None], pairs.shape)), name


def test_half_wave_lookups_hit_32_banks(images):
    sets, q = _data_sets()
    for name, v in sets:
        qq = np.broadcast_to(q[None, :], v.shape)
        for k, (addr, _, _) in enumerate(lookups(v, qq)):
            banks = (addr // 4) % 32
            assert (np.sort(banks, axis=1) == np.arange(32)[None, :]).all(), (name, k)


def test_step_equals_the_full_image_models(images):
    full, split = images
    w = split.view("<u4")
    model = KernelModelS4(full)
    sets, q = _data_sets()
    for name, v in sets:
        qq = np.broadcast_to(q[None, :], v.shape)
        got = np.zeros(v.shape, np.uint32)
        for addr, _, _ in lookups(v, qq):
            got ^= w[addr // 4]
        assert np.array_equal(got, model.s(v, qq)), name


def test_block_lin_through_the_split_image(images):
    """A whole block: three chained steps per lane from the split image, then
    the N_q lookups at their new offset, equal KernelModelS4.block_lin."""
    full, split = images
    w = split.view("<u4")
    model = KernelModelS4(full)
    rng = np.random.default_rng(7)
    blocks = rng.integers(0, 256, size=(24, 512), dtype=np.uint8)
    d = np.ascontiguousarray(blocks).view("<u4").reshape(-1, 32, 4)
    q = np.broadcast_to(np.arange(32)[None, :], d.shape[:2])

    def s(v):
        r = np.zeros(v.shape, np.uint32)
        for addr, _, _ in lookups(v, q):
            r ^= w[addr // 4]
        return r

    u = s(s(s(d[..., 0]) ^ d[..., 1]) ^ d[..., 2]) ^ d[..., 3]
    acc = np.zeros(u.shape, np.uint32)
    for t in range(8):
        n = ((u >> (4 * t)) & 15).astype(np.int64)
        acc ^= w[(NIB_OFF + (t >> 1) * 4096 + n * 256 + (t & 1) * 128 + q * 4) // 4]
    assert np.array_equal(np.bitwise_xor.reduce(acc, axis=1).astype(np.uint32), model.block_lin(blocks))
