"""Composite CRCs on the GPU (include/hdfs_crc32c.h section 6c;
csrc/crc32c_composite.hip): crc32c_composite_cells,
crc32c_composite_block_list and crc32c_plan_exec_blocks_composite.  Expected
values: the CRC of the bytes themselves where there are bytes (the oracle for
CRC32C, the reference's crc32c() too where its build exists, zlib.crc32 for
CRC32C_TYPE_CRC32), and the host crc32c_block_composite (checked against the
same oracles in tests/test_composite_host.py) where the checksums are random
words.  All results are bit-exact.  In every test the checksum arrays sit
inside a device buffer filled with 0xA5, and the output words sit between
guard words that must come back unchanged.  Sizes are placed from the
kernel's geometry hook, not hard-coded."""
from __future__ import annotations

import errno
import os
import zlib

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

BE = 0x1     # CRC32C_BIG_ENDIAN
CRC32 = 0x2  # CRC32C_TYPE_CRC32
GUARD = 0xEE
GUARD_WORDS = 8


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X (cuda:0)"
    return torch


class SumsBuffer:
    """A device buffer of 0xA5 bytes with checksum arrays written into it."""

    def __init__(self, nbytes: int):
        torch = _torch()
        self.t = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        self.base = self.t.data_ptr()
        assert self.base % 16 == 0

    def put(self, byte_off: int, words: np.ndarray) -> int:
        """Writes the words as stored (native u32) at byte_off; returns the device address."""
        torch = _torch()
        words = np.ascontiguousarray(words, np.uint32)
        assert byte_off % 4 == 0 and byte_off + words.nbytes <= self.t.numel()
        if words.size:
            self.t[byte_off:byte_off + words.nbytes] = torch.from_numpy(words.view(np.uint8).copy()).cuda()
        return self.base + byte_off


class CrcBuffer:
    """n output words between two runs of guard words, `phase` words past a 16-byte boundary."""

    def __init__(self, n: int, fill: int = GUARD, phase: int = 0):
        torch = _torch()
        self.n, self.fill, self.lead = n, fill, GUARD_WORDS + phase
        self.t = torch.full((4 * (n + 2 * GUARD_WORDS + 4),), fill, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * self.lead

    def read(self, flags: int = 0) -> np.ndarray:
        """The values (wire-order words swapped back with CRC32C_BIG_ENDIAN); asserts both guards intact."""
        _torch().cuda.synchronize()
        h = self.t.cpu().numpy()
        lo, hi = 4 * self.lead, 4 * (self.lead + self.n)
        assert (h[:lo] == self.fill).all(), "bytes before the outputs were written"
        assert (h[hi:] == self.fill).all(), "bytes after the outputs were written"
        w = h[lo:hi].copy().view(np.uint32)
        return w.byteswap() if flags & BE else w

    def untouched(self) -> bool:
        _torch().cuda.synchronize()
        return bool((self.t.cpu().numpy() == self.fill).all())


def _rand(rng, n) -> np.ndarray:
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _stored(sums: np.ndarray, flags: int) -> np.ndarray:
    return sums.byteswap() if flags & BE else sums


def _host(hdfs, sums, bpc, last_len, flags=0) -> int:
    """The host path over host-order values (the polynomial from flags)."""
    return hdfs.block_composite(sums, bpc, last_len, flags & CRC32) if len(sums) else 0


def _check(got, want, what=""):
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: outputs %s of %d differ (first: got %08x, want %08x)" % (
        what, bad[:10].tolist(), want.size, got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def geom(hdfs):
    g = hdfs.debug_composite_geometry()
    assert g["split_above"] == g["run"] * g["lanes"] + 1
    return g


@pytest.fixture(scope="module")
def crc_of(orc):
    ref = oracle.Reference() if os.path.exists(oracle.REF_SO) else None

    def castagnoli(data) -> int:
        a = np.ascontiguousarray(data, np.uint8)
        v = orc.crc32c(a)
        if ref is not None:
            assert ref.crc32c(a) == v
        return v

    def pick(flags):
        return (lambda d: zlib.crc32(np.ascontiguousarray(d, np.uint8).tobytes()) & 0xFFFFFFFF) if flags & CRC32 \
            else castagnoli

    return pick


# ---- 1. every geometry boundary, one list call per flag set -----------------
def boundary_sizes(g):
    seg = g["run"] * g["lanes"]
    wg = g["waves_per_workgroup"] * seg
    ns = [0, 1, 2, 63, 64, 65, seg - 1, seg, seg + 1]
    ns += [g["split_above"] - 1, g["split_above"], g["split_above"] + 1]  # one wave | two
    ns += [2 * seg, 2 * seg + 1, 2 * seg + 2]                              # two waves | three
    ns += [wg, wg + 1, wg + 2]                                             # one workgroup | two
    return sorted(set(ns))


@pytest.mark.parametrize("flags", [0, BE, CRC32, BE | CRC32])
def test_geometry_boundaries(hdfs, gpu_ctx, geom, flags):
    """n = 0, 1, 2, around a wave's lanes, around a full segment, around the
    split over waves and over workgroups, each with last_len 1 and bpc, in ONE
    list call; the n == 0 entries are NULL pointers."""
    bpc = 512
    rng = np.random.default_rng(100 + flags)
    ns, lasts, arrays = [], [], []
    for n in boundary_sizes(geom):
        for last in (1, bpc):
            ns.append(n)
            lasts.append(last)
            arrays.append(_rand(rng, n))
    buf = SumsBuffer(64 + sum(a.nbytes + 16 for a in arrays))
    ptrs, off = [], 64
    for a in arrays:
        ptrs.append(buf.put(off, _stored(a, flags)) if a.size else 0)
        off += a.nbytes + 16
    out = CrcBuffer(len(ns))
    gpu_ctx.composite_block_list(ptrs, ns, lasts, bpc, out.ptr, flags)
    want = [_host(hdfs, a, bpc, l, flags) for a, l in zip(arrays, lasts)]
    _check(out.read(flags), want, "n = %s" % ns)
    assert want[0] == want[1] == 0
    # small cells only: the launch that stores instead of accumulating
    small = [i for i, n in enumerate(ns) if n <= geom["split_above"]]
    out2 = CrcBuffer(len(small))
    gpu_ctx.composite_block_list([ptrs[i] for i in small], [ns[i] for i in small], [lasts[i] for i in small], bpc,
                                 out2.ptr, flags)
    _check(out2.read(flags), [want[i] for i in small], "small cells")


# ---- 2. contiguous form, many cells -----------------------------------------
@pytest.mark.parametrize("bpc", [1, 512, 700])
@pytest.mark.parametrize("cpc", [1, 7, 128, 2048])
def test_contiguous_many_cells(hdfs, gpu_ctx, cpc, bpc):
    """1, 63, 64, 65 and 257 cells; the last cell whole, of a single checksum
    and one checksum short; the array's last chunk 1 byte or bpc bytes."""
    rng = np.random.default_rng(200 + cpc + bpc)
    k = 0
    for ncells in (1, 63, 64, 65, 257):
        for tail in sorted({cpc, 1, max(cpc - 1, 1)}):
            n = (ncells - 1) * cpc + tail
            last_len = (1, bpc)[k % 2]
            k += 1
            sums = _rand(rng, n)
            buf = SumsBuffer(64 + sums.nbytes + 64)
            addr = buf.put(64, sums)
            assert hdfs.md5_nblocks(n, cpc) == ncells
            out = CrcBuffer(ncells)
            gpu_ctx.composite_cells(addr, n, cpc, bpc, last_len, out.ptr)
            want = [_host(hdfs, sums[i * cpc:(i + 1) * cpc], bpc, last_len if i == ncells - 1 else bpc)
                    for i in range(ncells)]
            _check(out.read(), want, "cpc %d, %d cells, last of %d, last_len %d" % (cpc, ncells, tail, last_len))


# ---- 3. both polynomials, from the bytes ------------------------------------
@pytest.mark.parametrize("flags", [0, CRC32, BE | CRC32])
def test_both_polynomials_from_bytes(hdfs, gpu_ctx, orc, crc_of, flags):
    """Chunk checksums made by the oracle (zlib.crc32 for CRC32: none of this
    library's code is in the expected value), stripe cells of 16 checksums of
    700 bytes, the last cell ragged with a 123-byte last chunk."""
    bpc, cpc = 700, 16
    data = oracle.xorshift64_bytes(100 * bpc + 123, 31337)
    chunks = [data[o:o + bpc] for o in range(0, data.size, bpc)]
    crc = crc_of(flags)
    sums = np.array([crc(c) for c in chunks], np.uint32)
    buf = SumsBuffer(64 + sums.nbytes + 64)
    addr = buf.put(64, _stored(sums, flags))
    ncells = -(-sums.size // cpc)
    out = CrcBuffer(ncells)
    gpu_ctx.composite_cells(addr, sums.size, cpc, bpc, 123, out.ptr, flags)
    want = [crc(data[i * cpc * bpc:(i + 1) * cpc * bpc]) for i in range(ncells)]
    got = out.read(flags)
    _check(got, want)
    lens = [min(cpc * bpc, data.size - i * cpc * bpc) for i in range(ncells)]
    assert hdfs.file_composite(got, lens, flags & CRC32) == crc(data)


# ---- 4. one large cell --------------------------------------------------------
@pytest.fixture(scope="module")
def large_cell(hdfs):
    sums = _rand(np.random.default_rng(400), 262144)
    sums.setflags(write=False)
    return sums, hdfs.block_composite(sums, 512, 512), hdfs.block_composite(sums, 512, 77)


def test_one_large_cell(hdfs, gpu_ctx, large_cell):
    """262 144 checksums (a 128 MiB block at bpc 512) as one cell: split over
    32 waves in 8 workgroups; contiguous and list form."""
    sums, want512, want77 = large_cell
    buf = SumsBuffer(64 + sums.nbytes + 64)
    addr = buf.put(64, sums)
    out = CrcBuffer(1)
    gpu_ctx.composite_cells(addr, sums.size, sums.size, 512, 512, out.ptr)
    _check(out.read(), [want512])
    out = CrcBuffer(2)
    gpu_ctx.composite_block_list([addr, addr], [sums.size] * 2, [77, 512], 512, out.ptr)
    _check(out.read(), [want77, want512])


def test_cold_state(hdfs, gpu_ctx, large_cell):
    """The same call straight after every CU's LDS was poisoned, on the same
    stream: the table is built from nothing an earlier launch left behind."""
    torch = _torch()
    sums, want512, _ = large_cell
    s = torch.cuda.Stream()
    buf = SumsBuffer(64 + sums.nbytes + 64)
    addr = buf.put(64, sums)
    out, out2 = CrcBuffer(1), CrcBuffer(32)
    torch.cuda.synchronize()
    assert hdfs.debug_lds_poison(0xC01DC0DE, s.cuda_stream) > 0
    gpu_ctx.composite_cells(addr, sums.size, sums.size, 512, 512, out.ptr, 0, s.cuda_stream)
    assert hdfs.debug_lds_poison(0x0DDBA11, s.cuda_stream) > 0
    gpu_ctx.composite_cells(addr, sums.size, 8192, 512, 512, out2.ptr, 0, s.cuda_stream)
    _check(out.read(), [want512])
    _check(out2.read(), [_host(hdfs, sums[i * 8192:(i + 1) * 8192], 512, 512) for i in range(32)])


# ---- 5. alignment ------------------------------------------------------------
def test_every_address_phase(hdfs, gpu_ctx, geom):
    """Inputs 0, 4, 8 and 12 bytes past a 16-byte boundary (an odd
    crc_per_cell moves every cell to another phase as well), outputs at every
    word phase; contiguous and list form, one split cell among the list's."""
    rng = np.random.default_rng(500)
    sums = _rand(rng, 37 * 70 - 5)
    big = _rand(rng, geom["split_above"] + 3)
    for in_phase in range(4):
        for out_phase in range(4):
            buf = SumsBuffer(64 + sums.nbytes + big.nbytes + 128)
            addr = buf.put(64 + 4 * in_phase, sums)
            out = CrcBuffer(70, phase=out_phase)
            gpu_ctx.composite_cells(addr, sums.size, 37, 700, 3, out.ptr)
            want = [_host(hdfs, sums[i * 37:(i + 1) * 37], 700, 3 if i == 69 else 700) for i in range(70)]
            _check(out.read(), want, "phases %d / %d" % (in_phase, out_phase))
            baddr = buf.put(64 + sums.nbytes + 32 + 4 * in_phase, big)
            ptrs = [addr + 4 * j for j in range(4)] + [baddr]
            ns = [33, 34, 35, 36, big.size]
            out = CrcBuffer(5, phase=out_phase)
            gpu_ctx.composite_block_list(ptrs, ns, [700] * 5, 700, out.ptr)
            want = [_host(hdfs, sums[j:j + 33 + j], 700, 700) for j in range(4)] + [_host(hdfs, big, 700, 700)]
            _check(out.read(), want, "list, phases %d / %d" % (in_phase, out_phase))


# ---- 6. more list entries than one launch holds -------------------------------
def test_more_than_the_launch_cap(hdfs, gpu_ctx):
    n = 2 * hdfs.COMPOSITE_LIST_MAX_BLOCKS + 1
    rng = np.random.default_rng(600)
    sums = _rand(rng, n * 20).reshape(n, 20)
    buf = SumsBuffer(64 + sums.nbytes + 64)
    base = buf.put(64, sums.reshape(-1))
    lasts = [1 + (i % 512) for i in range(n)]
    out = CrcBuffer(n)
    gpu_ctx.composite_block_list([base + 80 * i for i in range(n)], [20] * n, lasts, 512, out.ptr, BE)
    # (the words are host-order values read as wire order: the same as their swapped values)
    _check(out.read(BE), [_host(hdfs, r.byteswap(), 512, l) for r, l in zip(sums, lasts)])


# ---- 7. end to end on real payload ----------------------------------------------
def _block_packets(hdfs, blen, bpc, packet=65536):
    rows, pos, idx = [], 0, 0
    for plen in hdfs.packetize(blen, 0, packet, bpc):
        if plen:
            rows.append((pos, idx, plen, bpc))
            pos += plen
            idx += -(-plen // bpc)
    return np.array(rows, dtype=hdfs.PACKET_DTYPE), idx


@pytest.fixture(scope="module")
def stream_bytes():
    d = oracle.xorshift64_bytes(4 * 1024 * 1024 + 33 * 64 + 64, 7000)
    d.setflags(write=False)
    return d


@pytest.mark.parametrize("nblocks", [3, 33])
@pytest.mark.parametrize("blen", [4 * 1024 * 1024, 1024 * 1024 + 300])
def test_exec_blocks_composite_end_to_end(hdfs, gpu_ctx, crc_of, stream_bytes, blen, nblocks):
    """Blocks of real payload (block i = the stream from byte 64 i on) through
    exec_blocks_composite: every block CRC equals the oracle's CRC of the
    block's bytes, file_composite the oracle's CRC of all of them."""
    torch = _torch()
    crc = crc_of(0)
    pk, n = _block_packets(hdfs, blen, 512)
    blocks = [stream_bytes[64 * i:64 * i + blen] for i in range(nblocks)]
    dpays = [torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda() for b in blocks]
    stride = 4 * n + 16
    buf = SumsBuffer(64 + stride * nblocks)
    outs = [buf.base + 64 + stride * i for i in range(nblocks)]
    out = CrcBuffer(nblocks)
    plan = gpu_ctx.plan(pk, 0)
    assert plan.composite_shape() == (512, blen % 512 or 512)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.exec_blocks_composite([d.data_ptr() for d in dpays], outs, out.ptr, s.cuda_stream)
    got = out.read()
    plan.close()
    _check(got, [crc(b) for b in blocks])
    assert hdfs.file_composite(got, [blen] * nblocks) == crc(np.concatenate(blocks))
    h = buf.t.cpu().numpy()
    for i in range(nblocks):  # nothing around the checksum arrays
        assert (h[64 + stride * i + 4 * n:64 + stride * (i + 1)] == 0xA5).all()


def test_same_payload_under_every_bpc(hdfs, gpu_ctx, crc_of, stream_bytes):
    """1 MiB through plans of bpc 512, 1024, 4096, 700 and 1000 (wire-order
    checksums): exec, then composite_cells with one cell, on one stream.  All
    five composites are equal and are the oracle's CRC of the megabyte."""
    torch = _torch()
    data = stream_bytes[:1 << 20]
    dpay = torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), data, np.zeros(16, np.uint8)])).cuda()
    s = torch.cuda.Stream()
    got = []
    for bpc in (512, 1024, 4096, 700, 1000):
        # packets of 64 whole chunks (a DataNode's packets are whole chunks but for a block's last)
        rows = [(pos, pos // bpc, min(64 * bpc, data.size - pos), bpc) for pos in range(0, data.size, 64 * bpc)]
        pk, n = np.array(rows, dtype=hdfs.PACKET_DTYPE), -(-data.size // bpc)
        plan = gpu_ctx.plan(pk, BE)
        assert plan.nchecksums == n
        sbpc, last = plan.composite_shape()
        assert (sbpc, last) == (bpc, data.size % bpc or bpc)
        buf = SumsBuffer(64 + 4 * n + 64)
        out = CrcBuffer(1)
        torch.cuda.synchronize()
        plan.exec(dpay.data_ptr() + 16, buf.base + 64, s.cuda_stream)
        gpu_ctx.composite_cells(buf.base + 64, n, n, bpc, last, out.ptr, BE, s.cuda_stream)
        got.append(int(out.read(BE)[0]))
        plan.close()
    assert got == [crc_of(0)(data)] * 5, [hex(g) for g in got]


# ---- 8. plan_exec + composite_cells, stripe cells, no host sync between -----------
@pytest.mark.parametrize("flags", [BE, CRC32])
def test_plan_exec_then_stripe_cells(hdfs, gpu_ctx, crc_of, stream_bytes, flags):
    """A plan over 1 MiB + 70 000 bytes (64 KiB packets, bpc 512), then the
    CRC of every 64 KiB stripe cell (128 checksums) on the same stream."""
    torch = _torch()
    crc = crc_of(flags)
    data = stream_bytes[5:5 + (1 << 20) + 70000]
    pk, n = _block_packets(hdfs, data.size, 512)
    dpay = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()
    plan = gpu_ctx.plan(pk, flags)
    bpc, last = plan.composite_shape()
    assert (bpc, last) == (512, data.size % 512)
    buf = SumsBuffer(64 + 4 * n + 64)
    ncells = -(-n // 128)
    out = CrcBuffer(ncells)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.exec(dpay.data_ptr(), buf.base + 64, s.cuda_stream)
    gpu_ctx.composite_cells(buf.base + 64, n, 128, bpc, last, out.ptr, flags, s.cuda_stream)
    got = out.read(flags)
    plan.close()
    _check(got, [crc(data[i * 65536:(i + 1) * 65536]) for i in range(ncells)])
    lens = [min(65536, data.size - 65536 * i) for i in range(ncells)]
    assert hdfs.file_composite(got, lens, flags & CRC32) == crc(data)


# ---- 9. a buffers plan with an unaligned blockoffset -------------------------------
def test_buffers_plan_unaligned_blockoffset(hdfs, gpu_ctx, crc_of, stream_bytes):
    """crc32c_plan_create_buffers at blockoffset 300: the first packet is the
    212 bytes up to the chunk boundary, the last chunk is short too."""
    torch = _torch()
    length = 3 * 65536 + 1000
    data = stream_bytes[9:9 + length]
    dpay = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).cuda()
    plan = gpu_ctx.write_plan([(dpay.data_ptr(), length)], 0, length, blockoffset=300, packetsize=65536, bpc=512)
    assert plan.composite_shape() == (512, (300 + length) % 512)
    n = plan.nchecksums
    buf = SumsBuffer(64 + 4 * n + 64)
    out = CrcBuffer(1)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.exec(0, buf.base + 64, s.cuda_stream)
    gpu_ctx.composite_cells(buf.base + 64, n, n, 512, (300 + length) % 512, out.ptr, 0, s.cuda_stream)
    got = out.read()
    plan.close()
    _check(got, [crc_of(0)(data)])


# ---- 10. plans of and not of the shape ----------------------------------------------
def test_plan_shapes(hdfs, gpu_ctx):
    """composite_shape through crc32c_plan_create; a plan not of the shape is
    refused by exec_blocks_composite, which then launches nothing."""
    torch = _torch()

    def pk(rows):
        return np.array(rows, dtype=hdfs.PACKET_DTYPE)

    accepted = [
        (oracle.uniform_packets(4, 65536, 512), (512, 512)),
        (pk([(0, 0, 65536, 512), (65536, 128, 1000, 512), (66536, 130, 0, 512)]), (512, 488)),
        (pk([(0, 0, 300, 512), (300, 1, 65536, 512), (65836, 129, 5, 512)]), (512, 5)),
    ]
    for rows, want in accepted:
        plan = gpu_ctx.plan(rows)
        assert plan.composite_shape() == want
        plan.close()
    refused = [
        oracle.mixed_packets(6),                                                   # mixed bpc
        pk([(0, 0, 1024, 512), (1024, 2, 100, 512), (1124, 3, 1024, 512)]),        # a short packet in the middle
        pk([(0, 0, 1024, 512), (1024, 3, 1024, 512)]),                             # an out_idx gap
    ]
    pay = torch.zeros(6 * 65536 + 16, dtype=torch.uint8, device="cuda")
    for rows in refused:
        plan = gpu_ctx.plan(rows)
        with pytest.raises(hdfs.Crc32cError) as e:
            plan.composite_shape()
        assert e.value.rc == -errno.EINVAL
        n = plan.nchecksums
        sums = SumsBuffer(64 + 4 * n + 64)
        out = CrcBuffer(1, fill=0x77)
        with pytest.raises(hdfs.Crc32cError) as e:
            plan.exec_blocks_composite([pay.data_ptr()], [sums.base + 64], out.ptr)
        assert e.value.rc == -errno.EINVAL
        assert out.untouched()
        torch.cuda.synchronize()
        assert (sums.t.cpu().numpy() == 0xA5).all(), "a refused exec_blocks_composite launched its checksums"
        plan.exec(pay.data_ptr(), sums.base + 64)  # the plan behaves as before everywhere else
        torch.cuda.synchronize()
        assert not (sums.t.cpu().numpy()[64:64 + 4 * n] == 0xA5).all()
        plan.close()


# ---- 11. graph capture -------------------------------------------------------------
def test_graph_capture_three_replays(hdfs, gpu_ctx, geom):
    """composite_cells over split cells (the clear of the output and the
    accumulating launch) and composite_block_list over small ones, captured on
    a side stream and replayed three times over changed inputs."""
    torch = _torch()
    cpc = geom["split_above"] + 1000
    n = 2 * cpc + 17
    rng = np.random.default_rng(1100)
    inputs = [_rand(rng, n) for _ in range(3)]
    buf = SumsBuffer(64 + 4 * n + 64)
    addr = buf.put(64, inputs[0])
    out, out2 = CrcBuffer(3), CrcBuffer(4)
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        gpu_ctx.composite_cells(addr, n, cpc, 512, 9, out.ptr, 0, cap.cuda_stream)
        gpu_ctx.composite_block_list([addr + 400 * j for j in range(4)], [100] * 4, [512, 1, 2, 3], 512, out2.ptr, 0,
                                     cap.cuda_stream)
    torch.cuda.synchronize()
    assert out.untouched() and out2.untouched(), "the capture itself ran the kernels"
    for r in range(3):
        buf.put(64, inputs[r])
        out.t.fill_(GUARD)
        out2.t.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        s = inputs[r]
        _check(out.read(), [_host(hdfs, s[i * cpc:(i + 1) * cpc], 512, 9 if i == 2 else 512) for i in range(3)],
               "replay %d" % r)
        _check(out2.read(), [_host(hdfs, s[100 * j:100 * j + 100], 512, l) for j, l in enumerate([512, 1, 2, 3])],
               "replay %d (list)" % r)
    del g


# ---- 12. argument errors --------------------------------------------------------------
def test_argument_errors(hdfs, gpu_ctx):
    """Every refused call raises Crc32cError(-EINVAL) and leaves a poisoned
    output untouched; empty inputs succeed and write nothing."""
    torch = _torch()
    sums = np.arange(64, dtype=np.uint32)
    buf = SumsBuffer(64 + sums.nbytes + 64)
    a = buf.put(64, sums)
    out = CrcBuffer(4, fill=0x77)
    d = out.ptr
    closed = hdfs.Context.__new__(hdfs.Context)
    closed.handle, closed.device = None, 0
    pk = oracle.uniform_packets(1, 65536, 512)
    pay = torch.zeros(65536 + 16, dtype=torch.uint8, device="cuda")
    outbuf = SumsBuffer(64 + 4 * 128 + 64)
    plan = gpu_ctx.plan(pk)
    cells, lst = gpu_ctx.composite_cells, gpu_ctx.composite_block_list
    refused = [
        ("other flag bit", lambda: cells(a, 64, 16, 512, 512, d, flags=0x4)),
        ("other flag bit (list)", lambda: lst([a], [16], [512], 512, d, flags=0x8)),
        ("NULL ctx", lambda: closed.composite_cells(a, 64, 16, 512, 512, d)),
        ("NULL ctx (list)", lambda: closed.composite_block_list([a], [16], [512], 512, d)),
        ("crc_per_cell 0", lambda: cells(a, 64, 0, 512, 512, d)),
        ("bpc 0", lambda: cells(a, 64, 16, 0, 0, d)),
        ("bpc 0 (list)", lambda: lst([a], [16], [1], 0, d)),
        ("last_len 0", lambda: cells(a, 64, 16, 512, 0, d)),
        ("last_len > bpc", lambda: cells(a, 64, 16, 512, 513, d)),
        ("last_len 0 (list)", lambda: lst([a, a], [16, 16], [512, 0], 512, d)),
        ("last_len > bpc (list)", lambda: lst([a], [16], [513], 512, d)),
        ("NULL array", lambda: cells(0, 64, 16, 512, 512, d)),
        ("NULL list entry with checksums", lambda: lst([a, 0], [16, 1], [512, 512], 512, d)),
        ("NULL dev_crcs", lambda: cells(a, 64, 16, 512, 512, 0)),
        ("NULL dev_crcs (list)", lambda: lst([a], [16], [512], 512, 0)),
        ("NULL dev_crcs (plan)", lambda: plan.exec_blocks_composite([pay.data_ptr()], [outbuf.base + 64], 0)),
        ("NULL output pointer", lambda: plan.exec_blocks_composite([pay.data_ptr()] * 2, [outbuf.base + 64, 0], d)),
        ("NULL payload pointer", lambda: plan.exec_blocks_composite([pay.data_ptr(), 0], [outbuf.base + 64] * 2, d)),
        ("array off 4-byte alignment", lambda: cells(a + 2, 32, 16, 512, 512, d)),
        ("list entry off 4-byte alignment", lambda: lst([a, a + 1], [16, 16], [512, 512], 512, d)),
        ("dev_crcs off 4-byte alignment", lambda: cells(a, 64, 16, 512, 512, d + 2)),
        ("dev_crcs off 4-byte alignment (list)", lambda: lst([a], [16], [512], 512, d + 1)),
        ("output off 4-byte alignment", lambda: plan.exec_blocks_composite([pay.data_ptr()], [outbuf.base + 66], d)),
    ]
    for what, call in refused:
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == -errno.EINVAL, what
    # empty inputs: 0, nothing written (also with NULL arrays)
    cells(0, 0, 16, 512, 512, d)
    lst([], [], [], 512, d)
    plan.exec_blocks_composite([], [], d)
    assert out.untouched()
    torch.cuda.synchronize()
    assert (outbuf.t.cpu().numpy() == 0xA5).all(), "a refused exec_blocks_composite launched its checksums"
    plan.close()
