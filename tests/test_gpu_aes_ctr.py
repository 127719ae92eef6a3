"""AES/CTR/NoPadding on the GPU (include/hdfs_crc32c.h section 7;
csrc/aes_ctr.hip): hdfs_aes_ctr_xor_strided_dev and hdfs_aes_ctr_xor_list_dev.
Expected bytes: the host path hdfs_aes_ctr_xor (checked against NIST and
OpenSSL in tests/test_aes_ctr_host.py) and the OpenSSL goldens
(tests/golden/aes_ctr.json).  All results are bit-exact.  In every test the
destinations sit in a device buffer of 0xEE, and the WHOLE buffer is compared
with its expected image, so every byte outside the segments must come back
unchanged.  Sizes are placed from the kernel's geometry hook."""
from __future__ import annotations

import errno
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0xEE
KEYS = {bits: bytes(range(0x40, 0x40 + bits // 8)) for bits in (128, 192, 256)}
IV = bytes(range(0xA0, 0xB0))


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X (cuda:0)"
    return torch


@pytest.fixture(scope="module")
def geom(hdfs):
    g = hdfs.debug_aes_geometry()
    assert g["list_max_segments"] == hdfs.AES_LIST_MAX_SEGMENTS >= 64
    assert g["lane_bytes"] % 16 == 0 and g["wave_bytes"] == 64 * g["lane_bytes"]
    assert g["workgroup_bytes"] % g["wave_bytes"] == 0 and g["lanes_per_cu"] % 64 == 0
    return g


@pytest.fixture(scope="module")
def data():
    d = oracle.xorshift64_bytes((1 << 20) + 4096, oracle.SEED)
    d.setflags(write=False)
    return d


class Dst:
    """A device buffer of 0xEE bytes (16-byte aligned) and its expected image on the host."""

    def __init__(self, nbytes: int):
        torch = _torch()
        self.t = torch.full((nbytes,), GUARD, dtype=torch.uint8, device="cuda")
        self.base = self.t.data_ptr()
        assert self.base % 16 == 0
        self.want = np.full(nbytes, GUARD, np.uint8)

    def expect(self, off: int, expected: np.ndarray) -> int:
        """Notes the bytes a call must leave at ``off``; returns the device address."""
        assert 0 <= off and off + expected.size <= self.want.size
        self.want[off:off + expected.size] = expected
        return self.base + off

    def reset(self):
        self.t.fill_(GUARD)
        self.want[:] = GUARD

    def check(self, what=""):
        _torch().cuda.synchronize()
        got = self.t.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, "%s: %d bytes differ, first at %d (got %02x, want %02x)" % (
            what, bad.size, bad[0], got[bad[0]], self.want[bad[0]])


def _dev(a: np.ndarray):
    """The bytes in device memory behind 16 bytes of slack each side; (tensor, address of byte 0)."""
    torch = _torch()
    t = torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), a, np.zeros(16, np.uint8)])).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 16


# ---- 1. the alignment cross ----------------------------------------------------------
def test_alignment_cross(hdfs, gpu_ctx, data):
    """All 16 x 16 x 16 combinations of src % 16, dst % 16 and stream_off % 16 through the list form,
    lengths cycling through 1, 15, 16, 17, 31, 47, 100 (seven of them: coprime to 16, so every length
    meets every value of every phase); every fifth segment at a stream offset below 16."""
    aes = hdfs.AesCtr(KEYS[128], IV)
    lens = (1, 15, 16, 17, 31, 47, 100)
    slot = 160
    n = 16 * 16 * 16
    src_t, src = _dev(data[:n * slot])
    dst = Dst(n * slot + 32)
    segs = []
    for i in range(n):
        sp, dp, op = i & 15, (i >> 4) & 15, (i >> 8) & 15
        ln = lens[i % len(lens)]
        so = op if i % 5 == 0 else ((i * 2654435761) % (1 << 44)) * 16 + op
        s_off, d_off = i * slot + sp, 16 + i * slot + dp
        want = aes.xor(so, data[s_off:s_off + ln])
        segs.append((src + s_off, dst.expect(d_off, want), so, ln))
        assert (segs[-1][0] % 16, segs[-1][1] % 16, so % 16) == (sp, dp, op)
    gpu_ctx.aes_ctr_xor_list(aes, segs)
    dst.check("alignment cross")


# ---- 2. around every geometry unit ----------------------------------------------------
@pytest.mark.parametrize("so_phase,dst_phase", [(0, 0), (9, 3)])
def test_unit_boundaries(hdfs, gpu_ctx, geom, data, so_phase, dst_phase):
    """len = m U + d for U in (lane, wave, workgroup), m in (1, 2), d in (-1, 0, 1), one contiguous
    call each; keystream phase 0 with everything aligned, and phase 9 with dst 3 bytes off."""
    aes = hdfs.AesCtr(KEYS[256], IV)
    sizes = [m * geom[u] + d for u in ("lane_bytes", "wave_bytes", "workgroup_bytes") for m in (1, 2)
             for d in (-1, 0, 1)]
    src_t, src = _dev(data[:max(sizes) + 16 * len(sizes)])
    pitch = (max(sizes) + 63) // 16 * 16
    dst = Dst(pitch * len(sizes) + 32)
    so = (1 << 36) + 16 * 1000 + so_phase
    for k, ln in enumerate(sizes):
        d = dst.expect(16 + k * pitch + dst_phase, aes.xor(so + 16 * k, data[16 * k:16 * k + ln]))
        gpu_ctx.aes_ctr_xor_strided(aes, src + 16 * k, d, ln, stream_off=so + 16 * k)
    dst.check("unit boundaries")


def test_windows_per_lane_thresholds(hdfs, gpu_ctx, geom):
    """A launch that cannot fill the device gives a lane 1 or 2 windows instead of lane_bytes / 16:
    lengths whose window count is exactly lanes_per_cu * CUs (one window per lane), one more (two),
    twice that (two) and one more (lane_bytes / 16), with src, dst and the stream all off phase."""
    torch = _torch()
    aes = hdfs.AesCtr(KEYS[128], IV)
    lanes = geom["lanes_per_cu"] * torch.cuda.get_device_properties(0).multi_processor_count
    big = oracle.xorshift64_bytes(32 * lanes + 64, oracle.SEED + 1)
    src_t, src = _dev(big)
    so = (1 << 45) + 9
    for windows in (lanes, lanes + 1, 2 * lanes, 2 * lanes + 1):
        ln = 16 * windows - 3  # dst 3 bytes past a boundary: exactly `windows` windows
        dst = Dst(ln + 64)
        d = dst.expect(16 + 3, aes.xor(so, big[6:6 + ln]))
        gpu_ctx.aes_ctr_xor_strided(aes, src + 6, d, ln, stream_off=so)
        dst.check("%d windows" % windows)


# ---- 2b. two and four windows per lane ---------------------------------------------------------
# A launch of more than lanes windows gives a lane 2 consecutive windows, one of more than 2 * lanes
# lane_bytes / 16 of them: the kernel then carries a keystream block and a source chunk from window to
# window, skips the extra block at keystream phase 0, and leaves the loop early where a segment ends
# inside a lane.  Every launch below is just over its threshold, and every test asserts through
# crc32c_debug_aes_*_launch_info -- the sizing the entry points launch from -- that it is.
WPL = pytest.mark.parametrize("mode", ["two", "full"])


def _wpl(geom, mode):
    return 2 if mode == "two" else geom["lane_bytes"] // 16


@pytest.fixture(scope="module")
def cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def lanes(geom, cus):
    assert geom["lane_bytes"] // 16 > 2
    return geom["lanes_per_cu"] * cus


def _threshold(lanes, wpl):
    """The most windows of a launch that still gives a lane fewer than wpl windows (wpl: 2, or lane_bytes / 16)."""
    return lanes * wpl // 2


@pytest.fixture(scope="module")
def big(geom, lanes):
    """Source bytes for a launch over the last threshold, on the host and (16-byte aligned) on the device."""
    b = oracle.xorshift64_bytes(16 * _threshold(lanes, geom["lane_bytes"] // 16) + 3 * 65536, oracle.SEED + 3)
    b.setflags(write=False)
    t, addr = _dev(b)
    return b, t, addr


def _strided_info(hdfs, cus, wpl, dst, seg_len, nsegs=1, dst_stride=0):
    info = hdfs.debug_aes_strided_launch_info(cus, dst, seg_len, nsegs, dst_stride)
    assert info["windows_per_lane"] == wpl, (info, wpl)
    return info


@pytest.fixture(scope="module")
def cross(hdfs, geom, data):
    """The small segments of the phase cross, relative to their buffers -- (src offset, dst offset, stream
    offset, length) -- and the expected image of their destination buffer.  With L = lane_bytes the lengths
    end in each of a lane's windows and one window into the next lane, at one dst phase or another."""
    L = geom["lane_bytes"]
    lens = (1, 15, 16, 17, 47, 100, L // 2 + 1, L - 16, L - 15, L, L + 1, 2 * L - 1, 2 * L + 2)
    assert len(set(lens)) == len(lens) and len(lens) % 2 == 1  # an odd count is coprime to 16
    slot = (max(lens) + 15 + 16) // 16 * 16
    n = 16 * 16 * 16
    assert n * slot + 16 <= data.size
    aes = hdfs.AesCtr(KEYS[128], IV)
    want = np.full(n * slot + 32, GUARD, np.uint8)
    segs, met = [], set()
    for i in range(n):
        sp, dp, op = i & 15, (i >> 4) & 15, (i >> 8) & 15
        ln = lens[i % len(lens)]
        so = op if i % 5 == 0 else ((i * 2654435761) % (1 << 44)) * 16 + op
        s_off, d_off = i * slot + sp, 16 + i * slot + dp
        want[d_off:d_off + ln] = aes.xor(so, data[s_off:s_off + ln])
        segs.append((s_off, d_off, so, ln))
        met |= {(ln, "src", sp), (ln, "dst", dp), (ln, "stream", op)}
    assert len(met) == len(lens) * 3 * 16  # every length meets every value of every phase
    want.setflags(write=False)
    return segs, want


@WPL
def test_alignment_cross_many_windows_per_lane(hdfs, gpu_ctx, geom, cus, lanes, data, big, cross, mode):
    """All 16 x 16 x 16 combinations of src % 16, dst % 16 and stream_off % 16 through list launches of 2
    and of lane_bytes / 16 windows per lane: list_max_segments - 3 small segments per launch (the most
    that leave room for the filler) and three filler segments of unequal length -- each many wave units
    and a ragged tail, at phases of its own, first, in the middle and last in the list, so the kernel's
    scan over first[] crosses multi-unit segments -- whose windows alone are one more than the
    threshold.  The filler is compared on the device after every launch (and once on the host), the small
    segments' buffer whole on the host after the last."""
    torch = _torch()
    wpl = _wpl(geom, mode)
    aes = hdfs.AesCtr(KEYS[128], IV)
    small, want = cross
    big_b, big_t, big_addr = big
    src_t, src = _dev(data[:want.size])
    dst = Dst(want.size)
    dst.want[:] = want
    over = _threshold(lanes, wpl) + 1
    counts = (over // 2, over // 3, over - over // 2 - over // 3)
    # src % 16, dst % 16, stream_off % 16, bytes the segment ends before its last window does
    shapes = ((5, 11, 2, 3), (0, 0, 0, 9), (7, 7, 12, 5))
    fill = Dst(16 * over + 16 * len(counts) + 32)
    fsegs, s_at, d_at = [], 0, 16
    for k, (nw, (sp, dp, op, short)) in enumerate(zip(counts, shapes)):
        ln = 16 * nw - dp - short
        so = ((k + 1) << 40) + op
        assert ln > 64 * geom["wave_bytes"] and s_at + sp + ln <= big_b.size
        d = fill.expect(d_at + dp, aes.xor(so, big_b[s_at + sp:s_at + sp + ln]))
        fsegs.append((big_addr + s_at + sp, d, so, ln))
        assert hdfs.debug_aes_list_launch_info(cus, fsegs[-1:])["windows"] == nw
        s_at, d_at = s_at + 16 * nw + 16, d_at + 16 * nw + 16
    fill_want = torch.from_numpy(fill.want).cuda()
    per = geom["list_max_segments"] - len(fsegs)
    slot_windows = (small[1][1] - small[0][1]) // 16 + 1
    for at in range(0, len(small), per):
        chunk = [(src + s, dst.base + d, so, ln) for s, d, so, ln in small[at:at + per]]
        segs = [fsegs[0]] + chunk[:per // 2] + [fsegs[1]] + chunk[per // 2:] + [fsegs[2]]
        assert len(segs) <= geom["list_max_segments"]
        info = hdfs.debug_aes_list_launch_info(cus, segs)
        assert info["windows_per_lane"] == wpl and over < info["windows"] <= over + per * slot_windows, info
        fill.t.fill_(GUARD)
        gpu_ctx.aes_ctr_xor_list(aes, segs)
        assert torch.equal(fill.t, fill_want), "the filler of the launch from segment %d on" % at
    fill.check("the filler")
    dst.check("alignment cross, %d windows per lane" % wpl)


# src % 16, dst % 16, stream_off % 16: keystream phase (stream_off - dst) % 16, source phase (src - dst) % 16
PHASE_CLASSES = {"aligned": (0, 0, 0), "source_off": (9, 5, 5), "keystream_off": (5, 5, 0), "both_off": (2, 13, 7)}


@WPL
@pytest.mark.parametrize("cls", list(PHASE_CLASSES))
def test_phase_classes_and_tails(hdfs, gpu_ctx, geom, cus, lanes, big, mode, cls):
    """Keystream phase and source phase each zero or not (all zero: src, dst and the stream offset on
    16-byte boundaries, what a block write is), one contiguous call per length: the threshold's windows
    and t more bytes, t ending 1 byte into, and at the end of, each of the next lane_bytes / 16 windows
    (at 2 windows per lane: both windows of the last lane and of one more)."""
    wpl = _wpl(geom, mode)
    sp, dp, op = PHASE_CLASSES[cls]
    assert (((op - dp) % 16 != 0), ((sp - dp) % 16 != 0)) == ("keystream" in cls or "both" in cls,
                                                             "source" in cls or "both" in cls)
    assert cls != "aligned" or (sp, dp, op) == (0, 0, 0)
    aes = hdfs.AesCtr(KEYS[128], IV)
    big_b, big_t, big_addr = big
    thr = _threshold(lanes, wpl)
    tails = [16 * k + d for k in range(geom["lane_bytes"] // 16) for d in (1, 16)]
    so = (1 << 45) + 16 * 77 + op
    top = 16 * thr - dp + max(tails)
    ref = aes.xor(so, big_b[sp:sp + top])  # (one keystream: a shorter call's bytes are its prefix)
    dst = Dst(16 + dp + top + 48)
    for t in tails:
        ln = 16 * thr - dp + t
        info = _strided_info(hdfs, cus, wpl, dst.base + 16 + dp, ln)
        assert info["windows"] == thr + (t + 15) // 16
        dst.reset()
        d = dst.expect(16 + dp, ref[:ln])
        gpu_ctx.aes_ctr_xor_strided(aes, big_addr + sp, d, ln, stream_off=so)
        dst.check("%s, %d windows per lane, %d bytes past the threshold" % (cls, wpl, t))


def test_strided_ragged_full_windows_per_lane(hdfs, gpu_ctx, geom, cus, lanes, big):
    """test_strided's ragged segments (no stride keeps a phase), just enough of them for lane_bytes / 16
    windows per lane: a lane's windows end inside it wherever a segment ends."""
    full = geom["lane_bytes"] // 16
    aes = hdfs.AesCtr(KEYS[192], IV)
    big_b, big_t, big_addr = big
    seg_len, ss, ds, sos = 1000, 1024, 1003, 1543
    so0 = (1 << 34) + 3
    per_seg = hdfs.debug_aes_strided_launch_info(cus, 21, seg_len, 2, ds)["windows"] // 2
    nsegs = _threshold(lanes, full) // per_seg + 1
    assert (nsegs - 1) * ss + seg_len <= big_b.size
    dst = Dst(nsegs * ds + 64)
    _strided_info(hdfs, cus, full, dst.base + 21, seg_len, nsegs, ds)
    assert hdfs.debug_aes_strided_launch_info(cus, dst.base + 21, seg_len, nsegs - 1, ds)["windows_per_lane"] < full
    for i in range(nsegs):
        dst.expect(21 + i * ds, aes.xor(so0 + i * sos, big_b[i * ss:i * ss + seg_len]))
    gpu_ctx.aes_ctr_xor_strided(aes, big_addr, dst.base + 21, seg_len, nsegs, ss, ds, so0, sos)
    dst.check("%d ragged segments" % nsegs)


def test_strided_packets_full_windows_per_lane(hdfs, gpu_ctx, geom, cus, lanes, big):
    """64 KiB packets with every address, stride and stream offset a multiple of 16 (keystream and source
    phase 0 in every segment), just enough of them for lane_bytes / 16 windows per lane; the destinations
    32 bytes apart, which must stay as they were."""
    full = geom["lane_bytes"] // 16
    aes = hdfs.AesCtr(KEYS[128], IV)
    big_b, big_t, big_addr = big
    seg_len, ss, ds, sos = 65536, 65536, 65536 + 32, 65536 + 48
    so0 = 1 << 36
    nsegs = _threshold(lanes, full) // (seg_len // 16) + 1
    assert nsegs > 1 and nsegs * ss <= big_b.size
    dst = Dst(nsegs * ds + 32)
    info = _strided_info(hdfs, cus, full, dst.base + 16, seg_len, nsegs, ds)
    assert info["windows"] == nsegs * (seg_len // 16)
    assert hdfs.debug_aes_strided_launch_info(cus, dst.base + 16, seg_len, nsegs - 1, ds)["windows_per_lane"] < full
    for i in range(nsegs):
        dst.expect(16 + i * ds, aes.xor(so0 + i * sos, big_b[i * ss:(i + 1) * ss]))
    gpu_ctx.aes_ctr_xor_strided(aes, big_addr, dst.base + 16, seg_len, nsegs, ss, ds, so0, sos)
    dst.check("%d aligned packets" % nsegs)


@WPL
@pytest.mark.parametrize("bits", [192, 256])
def test_key_sizes_many_windows_per_lane(hdfs, gpu_ctx, geom, cus, lanes, big, mode, bits):
    """AES-192 and AES-256 (builds of their own) one window over the threshold.  Everything aligned, with
    an IV whose carry from the low into the high 64 bits falls inside one lane -- after its 2nd of 4
    windows (its 1st of 2); and an IV of all ones at stream offset 2^63 + 7 with src and dst off phase."""
    wpl = _wpl(geom, mode)
    big_b, big_t, big_addr = big
    windows = _threshold(lanes, wpl) + 1
    lane = 64 * 37 + 41  # (lane 41 of wave unit 37)
    assert (lane + 1) * wpl <= windows
    first_block = 1000
    carried = first_block + lane * wpl + wpl // 2  # the first block whose counter has the carry
    iv = IV[:8] + ((1 << 64) - carried).to_bytes(8, "big")
    assert hdfs.AesCtr.counter(iv, carried - 1) == IV[:8] + b"\xff" * 8
    assert hdfs.AesCtr.counter(iv, carried) == (int.from_bytes(IV[:8], "big") + 1).to_bytes(8, "big") + bytes(8)
    ln = 16 * windows
    dst = Dst(ln + 64)
    aes = hdfs.AesCtr(KEYS[bits], iv)
    d = dst.expect(16, aes.xor(16 * first_block, big_b[:ln]))
    assert _strided_info(hdfs, cus, wpl, d, ln)["windows"] == windows
    gpu_ctx.aes_ctr_xor_strided(aes, big_addr, d, ln, stream_off=16 * first_block)
    dst.check("AES-%d, the carry in a lane of %d windows" % (bits, wpl))
    aes = hdfs.AesCtr(KEYS[bits], b"\xff" * 16)
    so = (1 << 63) + 7
    ln = 16 * windows - 3 - 5
    dst.reset()
    d = dst.expect(16 + 3, aes.xor(so, big_b[6:6 + ln]))
    assert _strided_info(hdfs, cus, wpl, d, ln)["windows"] == windows
    gpu_ctx.aes_ctr_xor_strided(aes, big_addr + 6, d, ln, stream_off=so)
    dst.check("AES-%d, an IV of all ones, %d windows per lane" % (bits, wpl))


def test_in_place_full_windows_per_lane(hdfs, gpu_ctx, geom, cus, lanes, big):
    """dst == src three bytes past a boundary, stream phase 13, one window over the last threshold: every
    lane reads the lane_bytes / 16 windows it writes.  Encrypt, then decrypt back to the plaintext."""
    full = geom["lane_bytes"] // 16
    aes = hdfs.AesCtr(KEYS[256], IV)
    big_b, big_t, big_addr = big
    n = 16 * (_threshold(lanes, full) + 1) - 3 - 6
    so = (1 << 50) + 13
    dst = Dst(n + 64)
    addr = dst.base + 19
    _strided_info(hdfs, cus, full, addr, n)
    dst.t[19:19 + n] = big_t[16:16 + n]
    dst.expect(19, aes.xor(so, big_b[:n]))
    gpu_ctx.aes_ctr_xor_strided(aes, addr, addr, n, stream_off=so)
    dst.check("encrypt in place")
    dst.expect(19, big_b[:n])
    gpu_ctx.aes_ctr_xor_strided(aes, addr, addr, n, stream_off=so)
    dst.check("decrypt in place")


# ---- 3. key sizes and counter carries ---------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_key_sizes_and_carries(hdfs, gpu_ctx, data, bits):
    """16 KiB segments: an IV whose low half ends ...ff00 (the carry into the high half falls 4 KiB
    in), an IV of all ones (the counter wraps after block 0), stream offsets 2^40 + 5 and 2^63."""
    n = 16384
    cases = [(IV[:8] + b"\xff" * 7 + b"\x00", 0), (b"\xff" * 16, 0), (IV, (1 << 40) + 5), (IV, 1 << 63),
             (b"\xff" * 16, (1 << 63) + 7)]
    src_t, src = _dev(data[:n + 16])
    dst = Dst((n + 64) * len(cases))
    for k, (iv, so) in enumerate(cases):
        aes = hdfs.AesCtr(KEYS[bits], iv)
        d = dst.expect(32 + k * (n + 64) + k, aes.xor(so, data[k:k + n]))
        gpu_ctx.aes_ctr_xor_strided(aes, src + k, d, n, stream_off=so)
    dst.check("AES-%d" % bits)


# ---- 4. the strided form ---------------------------------------------------------------
@pytest.mark.parametrize("nsegs", [1, 2, 65])
def test_strided(hdfs, gpu_ctx, data, nsegs):
    aes = hdfs.AesCtr(KEYS[192], IV)
    seg_len, ss, ds, sos = 1000, 1024, 1003, 1543
    so0 = (1 << 34) + 3
    src_t, src = _dev(data[:nsegs * ss])
    dst = Dst(nsegs * ds + 64)
    for i in range(nsegs):
        dst.expect(21 + i * ds, aes.xor(so0 + i * sos, data[i * ss:i * ss + seg_len]))
    gpu_ctx.aes_ctr_xor_strided(aes, src, dst.base + 21, seg_len, nsegs, ss, ds, so0, sos)
    dst.check("%d segments" % nsegs)


# ---- 5. more list entries than one launch holds ---------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_list_limit(hdfs, gpu_ctx, geom, data, extra):
    """HDFS_AES_LIST_MAX_SEGMENTS segments and one more, zero-length segments with NULL pointers
    among them (the first, the one at the launch boundary, one in the middle)."""
    aes = hdfs.AesCtr(KEYS[128], IV)
    n = geom["list_max_segments"] + extra
    src_t, src = _dev(data[:n * 700 + 5000])
    dst = Dst(n * 704 + 5200)
    segs = []
    for i in range(n):
        if i in (0, 17, geom["list_max_segments"] - 1):
            segs.append((0, 0, i, 0))
            continue
        # (one segment of more than a wave unit; its destination lies behind all the others)
        ln = 5000 if i == 3 else 1 + (i * 53) % 699
        d_off = n * 704 + 101 if i == 3 else 16 + i * 704 + (i % 16)
        so = (i << 20) + i
        segs.append((src + i * 700, dst.expect(d_off, aes.xor(so, data[i * 700:i * 700 + ln])), so, ln))
    gpu_ctx.aes_ctr_xor_list(aes, segs)
    dst.check("%d segments" % n)


# ---- 6. in place, and the round trip -----------------------------------------------------
def test_in_place_and_round_trip(hdfs, gpu_ctx, geom, data):
    aes = hdfs.AesCtr(KEYS[256], IV)
    n = 2 * geom["workgroup_bytes"] + 777
    so = (1 << 50) + 13
    dst = Dst(n + 64)
    addr = dst.base + 19
    torch = _torch()
    dst.t[19:19 + n] = torch.from_numpy(data[:n].copy()).cuda()
    dst.expect(19, aes.xor(so, data[:n]))
    gpu_ctx.aes_ctr_xor_strided(aes, addr, addr, n, stream_off=so)
    dst.check("encrypt in place")
    dst.expect(19, data[:n])
    gpu_ctx.aes_ctr_xor_strided(aes, addr, addr, n, stream_off=so)
    dst.check("decrypt in place")


# ---- 7. goldens --------------------------------------------------------------------------------
def test_goldens(hdfs, gpu_ctx, data):
    with open(os.path.join(GOLDEN, "aes_ctr.json")) as f:
        golden = json.load(f)["golden"]
    assert len(golden) == 3
    torch = _torch()
    src_t, src = _dev(data[:1 << 20])
    for g in golden:
        assert g["bytes"] == 1 << 20 and g["seed"] == oracle.SEED
        aes = hdfs.AesCtr(bytes.fromhex(g["key"]), bytes.fromhex(g["iv"]))
        out = torch.full(((1 << 20) + 32,), GUARD, dtype=torch.uint8, device="cuda")
        gpu_ctx.aes_ctr_xor_strided(aes, src, out.data_ptr() + 16, 1 << 20, stream_off=g["stream_off"])
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert hashlib.sha256(h[16:-16].tobytes()).hexdigest() == g["sha256"]
        assert (h[:16] == GUARD).all() and (h[-16:] == GUARD).all()


# ---- 8. cold LDS ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0xC01DC0DE, 0x0DDBA11])
def test_cold_lds(hdfs, gpu_ctx, geom, data, seed):
    """The launch straight after every CU's LDS was poisoned, on the same stream: the table is built
    from nothing an earlier launch left behind."""
    torch = _torch()
    aes = hdfs.AesCtr(KEYS[128], IV)
    n = 16 * geom["workgroup_bytes"] + 5
    src_t, src = _dev(data[:n])
    dst = Dst(n + 64)
    d = dst.expect(35, aes.xor(7, data[:n]))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert hdfs.debug_lds_poison(seed, s.cuda_stream) > 0
    gpu_ctx.aes_ctr_xor_strided(aes, src, d, n, stream_off=7, stream=s.cuda_stream)
    dst.check("after the poison")


# ---- 9. graph replay ----------------------------------------------------------------------------
def test_graph_replay(hdfs, gpu_ctx, data):
    """Both forms captured (the project's graphs.capture_agreed), out of place, replayed twice over
    changed inputs: the same calls, the same bytes."""
    from hdfs_crc32c_amd.graphs import capture_agreed

    torch = _torch()
    aes = hdfs.AesCtr(KEYS[192], IV)
    n = 40000
    src_t, src = _dev(data[:n])
    dst = Dst(2 * n + 128)
    a = dst.base + 16 + 5
    b = dst.base + 16 + n + 48
    segs = [(src + 100, b, 1 << 30, 3000), (0, 0, 0, 0), (src + 7, b + 3001, 77, 333)]
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()

    def capture():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            gpu_ctx.aes_ctr_xor_strided(aes, src, a, n, stream_off=(1 << 41) + 9, stream=cap.cuda_stream)
            gpu_ctx.aes_ctr_xor_list(aes, segs, stream=cap.cuda_stream)
        return g

    g, err = capture_agreed(capture, 1)
    assert g is not None, err
    dst.check("the capture itself ran the kernels")
    for r in range(2):
        inp = data[r * 1000:r * 1000 + n]
        src_t[16:16 + n] = torch.from_numpy(inp.copy()).cuda()
        dst.t.fill_(GUARD)
        dst.want[:] = GUARD
        dst.expect(21, aes.xor((1 << 41) + 9, inp))
        dst.expect(16 + n + 48, aes.xor(1 << 30, inp[100:3100]))
        dst.expect(16 + n + 48 + 3001, aes.xor(77, inp[7:340]))
        torch.cuda.synchronize()
        g.replay()
        dst.check("replay %d" % r)
    del g


# ---- 10. with the checksum path -------------------------------------------------------------------
def test_zone_order_encrypt_then_checksum(hdfs, gpu_ctx, orc, data):
    """An encryption-zone write: encrypt 4 packets of 64 KiB, then Plan.exec over the ciphertext on the
    same stream; the checksums are the oracle's over the host's ciphertext."""
    torch = _torch()
    aes = hdfs.AesCtr(KEYS[256], IV)
    pk = oracle.uniform_packets(4, 65536, 512)
    n = 4 * 65536
    file_off = 3 * (128 << 20) + 4096
    cipher = aes.xor(file_off, data[:n])
    src_t, src = _dev(data[:n])
    dst = Dst(n + 32)
    d = dst.expect(16, cipher)
    sums = torch.zeros(hdfs.total_checksums(pk), dtype=torch.int32, device="cuda")
    plan = gpu_ctx.plan(pk)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu_ctx.aes_ctr_xor_strided(aes, src, d, n, stream_off=file_off, stream=s.cuda_stream)
    plan.exec(d, sums.data_ptr(), s.cuda_stream)
    s.synchronize()
    dst.check("ciphertext")
    assert np.array_equal(sums.cpu().numpy().view(np.uint32), orc.batch(cipher, pk, sums.numel()))
    plan.close()


def test_wire_order_strided_data_segments(hdfs, gpu_ctx, orc, data):
    """An encrypted transfer: checksum, frame, then encrypt.  The data segments hdfs_aes_wire_segments
    reports for 4 uniform packets are one strided call (data 64 KiB apart in memory, 65536 + prefix
    apart in the stream); its output equals the data slices of the wire image encrypted as one stream
    on the host."""
    aes = hdfs.AesCtr(KEYS[128], IV)
    pk = oracle.uniform_packets(4, 65536, 512)
    n = 4 * 65536
    payload = data[5:5 + n]
    sums = orc.batch(payload, pk, hdfs.total_checksums(pk))
    prefixes, offs = hdfs.frame_packets(pk, sums)
    wire = b"".join(prefixes[int(offs[i]):int(offs[i + 1])] + payload[i * 65536:(i + 1) * 65536].tobytes()
                    for i in range(4))
    base = (1 << 32) + 9
    enc = aes.xor(base, wire)
    src_t, src = _dev(payload)
    dst = Dst(n + 32)
    pre, segs = hdfs.aes_wire_segments(pk, offs, base, src, dst.base + 16)
    stride = int(segs[1]["stream_off"]) - int(segs[0]["stream_off"])
    plen = int(offs[1])
    assert stride == 65536 + plen
    for i in range(4):
        assert (int(segs[i]["src"]), int(segs[i]["dst"]), int(segs[i]["len"])) == (
            src + i * 65536, dst.base + 16 + i * 65536, 65536)
        assert int(segs[i]["stream_off"]) == int(segs[0]["stream_off"]) + i * stride
        w = int(segs[i]["stream_off"]) - base
        dst.expect(16 + i * 65536, enc[w:w + 65536])
    gpu_ctx.aes_ctr_xor_strided(aes, int(segs[0]["src"]), int(segs[0]["dst"]), 65536, 4, 65536, 65536,
                                int(segs[0]["stream_off"]), stride)
    dst.check("wire data segments")
    # the same set through the list form
    dst.t.fill_(GUARD)
    gpu_ctx.aes_ctr_xor_list(aes, segs)
    dst.check("wire data segments (list)")


# ---- 11. argument errors ------------------------------------------------------------------------------
def test_argument_errors(hdfs, gpu_ctx, data):
    """Every refused call raises Crc32cError(-EINVAL) and launches nothing: the 0xEE buffers stay
    untouched.  Empty inputs succeed and write nothing."""
    aes = hdfs.AesCtr(KEYS[128], IV)
    bad_rounds = hdfs.AesCtr(KEYS[128], IV)
    bad_rounds.c.rounds = 11
    src_t, src = _dev(data[:4096])
    dst = Dst(8192)
    d = dst.base + 64
    closed = hdfs.Context.__new__(hdfs.Context)
    closed.handle, closed.device = None, 0
    st, ls = gpu_ctx.aes_ctr_xor_strided, gpu_ctx.aes_ctr_xor_list
    top = 1 << 64
    refused = [
        ("NULL ctx", lambda: closed.aes_ctr_xor_strided(aes, src, d, 100)),
        ("NULL ctx (list)", lambda: closed.aes_ctr_xor_list(aes, [(src, d, 0, 100)])),
        ("NULL hdfs_aes_ctr", lambda: st(None, src, d, 100)),
        ("NULL hdfs_aes_ctr (list)", lambda: ls(None, [(src, d, 0, 100)])),
        ("11 rounds", lambda: st(bad_rounds, src, d, 100)),
        ("11 rounds (list)", lambda: ls(bad_rounds, [(src, d, 0, 100)])),
        ("NULL src", lambda: st(aes, 0, d, 100)),
        ("NULL dst", lambda: st(aes, src, 0, 100)),
        ("NULL src in a list", lambda: ls(aes, [(src, d, 0, 100), (0, d + 200, 0, 1)])),
        ("NULL dst in a list", lambda: ls(aes, [(src, d, 0, 100), (src, 0, 0, 1)])),
        ("stream_off + len > 2^64", lambda: st(aes, src, d, 100, stream_off=top - 99)),
        ("stream_off + len > 2^64 (list)", lambda: ls(aes, [(src, d, 0, 100), (src, d + 200, top - 1, 2)])),
        ("the last segment's stream offset > 2^64", lambda: st(aes, src, d, 100, 3, 128, 128, top - 300, 128)),
        ("overlap, not equal", lambda: st(aes, d, d + 50, 100)),
        ("overlap, not equal (list)", lambda: ls(aes, [(src, d, 0, 100), (d + 300, d + 299, 0, 10)])),
    ]
    for what, call in refused:
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == -errno.EINVAL, what
        assert KEYS[128].hex()[:16] not in str(e.value), what
    # nothing to do: 0, nothing written, NULL pointers allowed
    st(aes, 0, 0, 0)
    st(aes, src, d, 100, nsegs=0)
    st(aes, src, d, 0, nsegs=5, dst_stride=16)
    ls(aes, [])
    ls(aes, [(0, 0, 5, 0), (0, 0, top - 1, 0)])
    dst.check("after refused and empty calls")
    # a stream that ends exactly at 2^64 is valid
    dst.expect(64, aes.xor(top - 100, data[:100]))
    st(aes, src, d, 100, stream_off=top - 100)
    dst.check("a stream ending at 2^64")
