"""Block MD5-of-CRCs on the GPU (include/hdfs_crc32c.h section 6b;
csrc/crc32c_md5.hip): crc32c_md5_blocks, crc32c_md5_block_list and
crc32c_plan_exec_blocks_md5 against hashlib.md5 over the checksums as
big-endian bytes.  In every test the checksum arrays sit inside a device
buffer filled with 0xA5, and the digest buffer carries 16 guard bytes before
and after its digests, which must come back unchanged."""
from __future__ import annotations

import errno
import hashlib

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

BE = 0x1  # CRC32C_BIG_ENDIAN
GUARD = 0xEE


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X (cuda:0)"
    return torch


def md5_of(sums: np.ndarray) -> bytes:
    """The expected digest of checksums given as host-order values."""
    return hashlib.md5(np.asarray(sums, np.uint32).astype(">u4").tobytes()).digest()


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


class DigestBuffer:
    """16 n digest bytes between two 16-byte guards."""

    def __init__(self, n: int, fill: int = GUARD):
        torch = _torch()
        self.n = n
        self.fill = fill
        self.t = torch.full((16 * n + 32,), fill, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + 16

    def read(self):
        """The digests; asserts that both guards are intact."""
        _torch().cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:16] == self.fill).all(), "bytes before the digests were written"
        assert (h[-16:] == self.fill).all(), "bytes after the digests were written"
        return [h[16 + 16 * i:32 + 16 * i].tobytes() for i in range(self.n)]

    def untouched(self) -> bool:
        _torch().cuda.synchronize()
        return bool((self.t.cpu().numpy() == self.fill).all())


def _check_digests(got, want, what=""):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, "%s: digests %s of %d differ" % (what, bad[:10], len(want))


def _run_contig(ctx, sums: np.ndarray, cpb: int, flags: int = 0, byte_off: int = 64, stream=0):
    """md5_blocks over `sums` (host-order values) stored at byte_off of a 0xA5 buffer."""
    stored = sums.byteswap() if flags & BE else sums
    buf = SumsBuffer(byte_off + sums.nbytes + 64)
    addr = buf.put(byte_off, stored)
    nb = -(-sums.size // cpb)
    dig = DigestBuffer(nb)
    ctx.md5_blocks(addr, sums.size, cpb, dig.ptr, flags, stream)
    want = [md5_of(sums[i * cpb:(i + 1) * cpb]) for i in range(nb)]
    return dig.read(), want


# ---- 1. padding boundaries -------------------------------------------------
PAD_NS = [0, 1, 2, 13, 14, 15, 16, 17, 29, 30, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("flags", [0, BE])
def test_padding_boundaries(hdfs, gpu_ctx, flags):
    """Every n mod 16 at which MD5's padding changes shape (0: a block of its
    own; 14, 15: the length spills into a second block), in one list call;
    host order and, on the byte-swapped arrays, CRC32C_BIG_ENDIAN give the
    same digests.  The n == 0 entry is a NULL pointer."""
    rng = np.random.default_rng(11)
    arrays = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in PAD_NS]
    buf = SumsBuffer(64 + sum(a.nbytes + 16 for a in arrays))
    ptrs, off = [], 64
    for a in arrays:
        ptrs.append(buf.put(off, a.byteswap() if flags else a) if a.size else 0)
        off += a.nbytes + 16
    dig = DigestBuffer(len(arrays))
    gpu_ctx.md5_block_list(ptrs, PAD_NS, dig.ptr, flags)
    _check_digests(dig.read(), [md5_of(a) for a in arrays], "n = %s" % PAD_NS)
    assert dig.read()[0] == hashlib.md5(b"").digest()


# ---- 2. wave and launch boundaries -----------------------------------------
@pytest.mark.parametrize("cpb", [1, 7, 16, 17, 128])
def test_wave_and_launch_boundaries(hdfs, gpu_ctx, cpb):
    """1, 63, 64, 65 and 257 blocks (a partial wave, a whole one, one lane into
    the next, several workgroups), the last block whole, one word short and
    one word long."""
    rng = np.random.default_rng(20 + cpb)
    for nblocks in (1, 63, 64, 65, 257):
        for short in sorted({0, 1, cpb - 1}):
            if short >= cpb:
                continue  # (cpb 1: the last block cannot lose a word)
            n = nblocks * cpb - short
            sums = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            got, want = _run_contig(gpu_ctx, sums, cpb)
            assert len(want) == nblocks == hdfs.md5_nblocks(n, cpb)
            _check_digests(got, want, "cpb %d, %d blocks, last short by %d" % (cpb, nblocks, short))


# ---- 3. alignment ----------------------------------------------------------
@pytest.mark.parametrize("byte_off", [4, 8, 12])
def test_alignment_contiguous(hdfs, gpu_ctx, byte_off):
    """The array 4, 8 and 12 bytes past a 16-byte boundary with an odd
    crc_per_block: every block then starts at another phase."""
    rng = np.random.default_rng(30 + byte_off)
    sums = rng.integers(0, 1 << 32, 37 * 70 - 5, dtype=np.uint64).astype(np.uint32)
    got, want = _run_contig(gpu_ctx, sums, 37, byte_off=64 + byte_off)
    _check_digests(got, want)


def test_alignment_list(hdfs, gpu_ctx):
    """List form, every array at a different offset from a 16-byte boundary."""
    rng = np.random.default_rng(34)
    ns = [37, 16, 33, 64, 1, 15, 100, 48]
    arrays = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in ns]
    buf = SumsBuffer(64 + sum(a.nbytes + 32 for a in arrays))
    ptrs, off = [], 64
    for k, a in enumerate(arrays):
        ptrs.append(buf.put(off + 4 * (k % 4), a))
        off += (a.nbytes + 32) & ~15
    assert {p % 16 for p in ptrs} == {0, 4, 8, 12}
    dig = DigestBuffer(len(ns))
    gpu_ctx.md5_block_list(ptrs, ns, dig.ptr)
    _check_digests(dig.read(), [md5_of(a) for a in arrays])


# ---- 4. the workload's block, 9. cold state --------------------------------
@pytest.fixture(scope="module")
def workload_sums():
    rng = np.random.default_rng(40)
    sums = rng.integers(0, 1 << 32, 3 * 8192 + 5000, dtype=np.uint64).astype(np.uint32)
    sums.setflags(write=False)
    want = [md5_of(sums[i * 8192:(i + 1) * 8192]) for i in range(4)]
    return sums, want


def test_workload_block(hdfs, gpu_ctx, workload_sums):
    """crc_per_block 8192 (a 4 MiB block of 512-byte chunks): 3 full blocks and one of 5000."""
    sums, want = workload_sums
    got, want2 = _run_contig(gpu_ctx, sums, 8192)
    assert want2 == want
    _check_digests(got, want)


def test_cold_state(hdfs, gpu_ctx, workload_sums):
    """The same call straight after every CU's LDS was poisoned, on the same
    stream: the kernel depends on nothing an earlier launch left behind."""
    torch = _torch()
    sums, want = workload_sums
    s = torch.cuda.Stream()
    buf = SumsBuffer(64 + sums.nbytes + 64)
    addr = buf.put(64, sums)
    dig = DigestBuffer(4)
    torch.cuda.synchronize()
    assert hdfs.debug_lds_poison(0xC01DC0DE, s.cuda_stream) > 0
    gpu_ctx.md5_blocks(addr, sums.size, 8192, dig.ptr, 0, s.cuda_stream)
    _check_digests(dig.read(), want)


# ---- 5. mixed lengths in one wave ------------------------------------------
def test_mixed_lengths_one_wave(hdfs, gpu_ctx):
    """64 arrays, short (0..40 words) and long (8000..8200) ones, their
    pointers in shuffled order: lanes of one wave with different trip counts
    and tails."""
    rng = np.random.default_rng(50)
    ns = [int(rng.integers(0, 41)) if rng.integers(0, 2) else int(rng.integers(8000, 8201)) for _ in range(64)]
    arrays = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in ns]
    buf = SumsBuffer(64 + sum(a.nbytes + 16 for a in arrays))
    ptrs, off = [], 64
    for a in arrays:
        ptrs.append(buf.put(off, a))
        off += a.nbytes + 16
    order = rng.permutation(64)
    dig = DigestBuffer(64)
    gpu_ctx.md5_block_list([ptrs[i] for i in order], [ns[i] for i in order], dig.ptr)
    _check_digests(dig.read(), [md5_of(arrays[i]) for i in order])


# ---- 6. more than the per-launch cap ---------------------------------------
def test_more_than_the_launch_cap(hdfs, gpu_ctx):
    """cap + 1 blocks of 20 words: a second launch carries the last block and
    writes its digest behind the first launch's."""
    n = hdfs.MD5_LIST_MAX_BLOCKS + 1
    rng = np.random.default_rng(60)
    sums = rng.integers(0, 1 << 32, (n, 20), dtype=np.uint64).astype(np.uint32)
    buf = SumsBuffer(64 + sums.nbytes + 64)
    base = buf.put(64, sums.reshape(-1))
    dig = DigestBuffer(n)
    gpu_ctx.md5_block_list([base + 80 * i for i in range(n)], [20] * n, dig.ptr)
    _check_digests(dig.read(), [md5_of(r) for r in sums])


# ---- 7. from the HIP path, no host sync between ----------------------------
def _file_packets(hdfs, block_lens, packet=65536, bpc=512):
    """hadoop_rpc_send_packets' packets of a file's blocks back to back, checksums packed."""
    rows, pos, idx = [], 0, 0
    for blen in block_lens:
        for plen in hdfs.packetize(blen, 0, packet, bpc):
            if plen:
                rows.append((pos, idx, plen, bpc))
                pos += plen
                idx += -(-plen // bpc)
    return np.array(rows, dtype=hdfs.PACKET_DTYPE), pos, idx


def test_plan_exec_then_md5_blocks(hdfs, gpu_ctx, orc):
    """7a: one CRC32C_BIG_ENDIAN plan over a file of four 256 KiB blocks and a
    last one of 100 000 bytes (64 KiB packets, bpc 512): exec, then md5_blocks
    with crc_per_block 512 on the same stream.  The digests equal hashlib's
    over the oracle's checksums in wire order, the file checksum too."""
    torch = _torch()
    pk, nbytes, n = _file_packets(hdfs, [262144] * 4 + [100000])
    assert n == 4 * 512 + 196
    payload = oracle.xorshift64_bytes(nbytes + 16, 707)
    wire = orc.batch(payload, pk, n, big_endian=True)
    want = [hashlib.md5(wire[i * 512:(i + 1) * 512].tobytes()).digest() for i in range(5)]
    dpay = torch.from_numpy(payload).cuda()
    buf = SumsBuffer(64 + 4 * n + 64)
    dig = DigestBuffer(5)
    plan = gpu_ctx.plan(pk, BE)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.exec(dpay.data_ptr(), buf.base + 64, s.cuda_stream)
    gpu_ctx.md5_blocks(buf.base + 64, n, 512, dig.ptr, BE, s.cuda_stream)
    got = dig.read()
    plan.close()
    _check_digests(got, want)
    assert hdfs.file_md5(b"".join(got)) == hashlib.md5(b"".join(want)).digest()
    assert [hdfs.block_md5(wire[i * 512:(i + 1) * 512], BE) for i in range(5)] == want  # (the host fallback agrees)


def _exec_blocks_md5_case(hdfs, ctx, orc, pk, nblocks, flags, seed):
    torch = _torch()
    n = hdfs.total_checksums(pk)
    blen = int((pk["payload_off"] + pk["len"]).max())
    pays = [oracle.xorshift64_bytes(blen + 16, seed + i) for i in range(nblocks)]
    dpays = [torch.from_numpy(p).cuda() for p in pays]  # (separate allocations)
    stride = 4 * n + 16
    buf = SumsBuffer(64 + stride * nblocks)
    outs = [buf.base + 64 + stride * i for i in range(nblocks)]
    dig = DigestBuffer(nblocks)
    plan = ctx.plan(pk, flags)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.exec_blocks_md5([d.data_ptr() for d in dpays], outs, dig.ptr, s.cuda_stream)
    got = dig.read()
    plan.close()
    want = [md5_of(orc.batch(p, pk, n)) for p in pays]
    _check_digests(got, want, "flags %d" % flags)
    # the checksums themselves, in the plan's order, and nothing around them
    h = buf.t.cpu().numpy()
    for i, p in enumerate(pays):
        o = 64 + stride * i
        assert np.array_equal(h[o:o + 4 * n].view(np.uint32), orc.batch(p, pk, n, big_endian=bool(flags & BE)))
        assert (h[o + 4 * n:o + stride] == 0xA5).all()


@pytest.mark.parametrize("flags", [0, BE])
def test_exec_blocks_md5_33_blocks(hdfs, gpu_ctx, orc, flags):
    """7b: 33 blocks of one 64 KiB packet each (more than one multi-block
    launch holds), payloads in separate allocations."""
    _exec_blocks_md5_case(hdfs, gpu_ctx, orc, oracle.uniform_packets(1, 65536, 512), 33, flags, 7100)


@pytest.mark.parametrize("flags", [0, BE])
def test_exec_blocks_md5_one_launch_per_block(hdfs, gpu_ctx, orc, flags):
    """7c: a block of 65 538 bytes: its 2-byte tail has no multi-block form, so
    the checksums run one launch per block."""
    pk = np.array([(0, 0, 65536, 512), (65536, 128, 2, 512)], dtype=hdfs.PACKET_DTYPE)
    _exec_blocks_md5_case(hdfs, gpu_ctx, orc, pk, 3, flags, 7200)


# ---- 8. graph capture ------------------------------------------------------
def test_graph_capture(hdfs, gpu_ctx, orc):
    """exec + md5_blocks of a two-block file captured on a side stream and
    replayed twice with the payload changed in between: the calls keep no
    host-side state, each replay digests what is in the payload then."""
    torch = _torch()
    pk, nbytes, n = _file_packets(hdfs, [131072, 131072])
    assert n == 512
    payloads = [oracle.xorshift64_bytes(nbytes + 16, 800 + r) for r in range(2)]
    dpay = torch.from_numpy(payloads[0]).cuda()
    buf = SumsBuffer(64 + 4 * n + 64)
    dig = DigestBuffer(2)
    plan = gpu_ctx.plan(pk, BE)
    cap = torch.cuda.Stream()
    plan.exec(dpay.data_ptr(), buf.base + 64, cap.cuda_stream)  # (the plan's upload is done before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        plan.exec(dpay.data_ptr(), buf.base + 64, cap.cuda_stream)
        gpu_ctx.md5_blocks(buf.base + 64, n, 256, dig.ptr, BE, cap.cuda_stream)
    torch.cuda.synchronize()
    assert dig.untouched(), "the capture itself ran the kernel"
    for r in range(2):
        dpay.copy_(torch.from_numpy(payloads[r]))
        dig.t.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        wire = orc.batch(payloads[r], pk, n, big_endian=True)
        _check_digests(dig.read(), [hashlib.md5(wire[i * 256:(i + 1) * 256].tobytes()).digest() for i in range(2)],
                       "replay %d" % r)
    del g
    plan.close()


# ---- 10. argument errors ---------------------------------------------------
def test_argument_errors(hdfs, gpu_ctx):
    """Every refused call raises Crc32cError(-EINVAL) and leaves a poisoned
    digest buffer untouched; empty inputs succeed and write nothing."""
    torch = _torch()
    sums = np.arange(64, dtype=np.uint32)
    buf = SumsBuffer(64 + sums.nbytes + 64)
    a = buf.put(64, sums)
    dig = DigestBuffer(4, fill=0x77)
    d = dig.ptr
    closed = hdfs.Context.__new__(hdfs.Context)
    closed.handle, closed.device = None, 0
    pk = oracle.uniform_packets(1, 65536, 512)
    pay = torch.zeros(65536 + 16, dtype=torch.uint8, device="cuda")
    outbuf = SumsBuffer(64 + 4 * 128 + 64)
    plan = gpu_ctx.plan(pk)
    refused = [
        ("other flag bit", lambda: gpu_ctx.md5_blocks(a, 64, 16, d, flags=0x2)),
        ("other flag bit (list)", lambda: gpu_ctx.md5_block_list([a], [16], d, flags=0x9)),
        ("NULL ctx", lambda: closed.md5_blocks(a, 64, 16, d)),
        ("NULL ctx (list)", lambda: closed.md5_block_list([a], [16], d)),
        ("crc_per_block 0", lambda: gpu_ctx.md5_blocks(a, 64, 0, d)),
        ("NULL array", lambda: gpu_ctx.md5_blocks(0, 64, 16, d)),
        ("NULL list entry with checksums", lambda: gpu_ctx.md5_block_list([a, 0], [16, 1], d)),
        ("NULL dev_md5", lambda: gpu_ctx.md5_blocks(a, 64, 16, 0)),
        ("NULL dev_md5 (list)", lambda: gpu_ctx.md5_block_list([a], [16], 0)),
        ("NULL dev_md5 (plan)", lambda: plan.exec_blocks_md5([pay.data_ptr()], [outbuf.base + 64], 0)),
        ("NULL output pointer", lambda: plan.exec_blocks_md5([pay.data_ptr()] * 2, [outbuf.base + 64, 0], d)),
        ("NULL payload pointer", lambda: plan.exec_blocks_md5([pay.data_ptr(), 0], [outbuf.base + 64] * 2, d)),
        ("array off 4-byte alignment", lambda: gpu_ctx.md5_blocks(a + 2, 32, 16, d)),
        ("list entry off 4-byte alignment", lambda: gpu_ctx.md5_block_list([a, a + 1], [16, 16], d)),
        ("dev_md5 off 4-byte alignment", lambda: gpu_ctx.md5_blocks(a, 64, 16, d + 2)),
        ("dev_md5 off 4-byte alignment (list)", lambda: gpu_ctx.md5_block_list([a], [16], d + 1)),
        ("output off 4-byte alignment", lambda: plan.exec_blocks_md5([pay.data_ptr()], [outbuf.base + 66], d)),
    ]
    for what, call in refused:
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == -errno.EINVAL, what
    # empty inputs: 0, nothing written (also with NULL arrays)
    gpu_ctx.md5_blocks(0, 0, 16, d)
    gpu_ctx.md5_blocks(a, 0, 0, d)
    gpu_ctx.md5_block_list([], [], d)
    plan.exec_blocks_md5([], [], d)
    assert dig.untouched()
    torch.cuda.synchronize()
    assert (outbuf.t.cpu().numpy() == 0xA5).all(), "a refused exec_blocks_md5 launched its checksums"
    plan.close()
