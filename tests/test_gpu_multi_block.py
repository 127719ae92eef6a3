"""Every production kernel build and every tile form in a multi-block launch
(crc32c_plan_exec_blocks and crc32c_plan_verify_blocks: one block's plan over
up to 32 blocks per launch, each block's payload and output offsets applied in
tile_at, csrc/crc32c_device.h).

The rows (multi_block_cases.py) are sized from the CU count; each first
asserts, through crc32c_debug_plan_blocks_launch_info, that every launch of
the call selects the kernel, the skip_z and the `general` bits the row names
and that the call does NOT fall back to one ordinary launch per block.  Then
exec_blocks writes every block's checksums into one shared array, in reverse
block order, with a guard word between blocks and at both ends: every block
must equal the oracle's checksums (zlib's for CRC32C_TYPE_CRC32) bit for bit
and every guard word must come back unchanged.  verify_blocks over the same
blocks must find clean data clean and report exactly the corruption set of
test_gpu_verify_blocks.py in verdicts, bitmap and per-launch results.  None of
this library's code is in the expected values; all comparisons are exact.

Each block holds data of its own in its own slot of one 0xA5-filled device
buffer; block addresses go up and down, so a launch's base is not its first
block's address."""
from __future__ import annotations

import numpy as np
import pytest

import multi_block_cases as mb
import oracle
from test_gpu_verify_blocks import Run, corruption

pytestmark = pytest.mark.gpu

LEAD = 32    # bytes of fill before a block's data in its slot (a multiple of 16)
OUT_FILL = 0x5A5A5A5A


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X (cuda:0)"
    return torch


class BlockSet:
    """The blocks of one shape: distinct data per block, block b in slot slot_of(b) of one device buffer
    filled with 0xA5, LEAD bytes into the slot or 5 bytes further (place()), and their expected checksums
    per checksum type (from the oracle / zlib).  Has what test_gpu_verify_blocks.Run takes."""

    def __init__(self, hdfs, gpu_ctx, orc, name):
        torch = _torch()
        self.hdfs, self.orc, self.name = hdfs, orc, name
        probe = gpu_ctx.plan(oracle.uniform_packets(1))
        self.num_cu = int(probe.launch_info(0x1000).num_cu)  # (the CU count launches are sized for)
        probe.close()
        s = mb.SHAPES[name]
        self.pk = mb.packets(s.shape, s.packets_at(self.num_cu))
        tiles, gen = hdfs.debug_plan(self.pk)
        assert tiles.size and not gen.size
        self.block_tiles = int(tiles.size)
        self.n = int(hdfs.total_checksums(self.pk))
        self.blen = int((self.pk["payload_off"] + self.pk["len"]).max())
        self.m = mb.max_blocks(name, self.num_cu, self.block_tiles)
        # a slot: LEAD bytes, the block (5 bytes further when off), up to the next 16-byte boundary and 64 more
        self.slot = LEAD + (self.blen + 5 + 15) // 16 * 16 + 64
        stream = oracle.xorshift64_bytes(self.blen + 64 * self.m, 0xB10C5 + sum(map(ord, name)))
        self.data = [stream[64 * b:64 * b + self.blen] for b in range(self.m)]
        assert not np.array_equal(self.data[0][:64], self.data[1][:64])
        self.t = torch.full((self.slot * self.m,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.skew = [None] * self.m
        self.off = [0] * self.m
        self._expected = {}
        self.place(set())

    def place(self, off_blocks):
        """Block b's data 5 bytes off 16-byte alignment for b in off_blocks, aligned otherwise."""
        torch = _torch()
        for b in range(self.m):
            skew = 5 if b in off_blocks else 0
            if self.skew[b] == skew:
                continue
            base = mb.slot_of(b, self.m) * self.slot
            self.t[base:base + self.slot] = 0xA5
            self.off[b] = base + LEAD + skew
            self.t[self.off[b]:self.off[b] + self.blen] = torch.from_numpy(self.data[b].copy()).cuda()
            self.skew[b] = skew
        torch.cuda.synchronize()
        self.ptrs = [self.t.data_ptr() + o for o in self.off]
        assert all((p % 16 == 5) == (b in off_blocks) and p % 16 in (0, 5) for b, p in enumerate(self.ptrs))

    def use_flags(self, flags):
        """self.expected: every block's checksums of this checksum type and byte order (computed once)."""
        if flags not in self._expected:
            if flags & mb.CRC32:
                exp = [_byte_order(oracle.zlib_batch(d, self.pk, self.n), flags) for d in self.data]
            else:
                exp = [self.orc.batch(d, self.pk, self.n, big_endian=bool(flags & mb.BE)) for d in self.data]
            e = np.stack(exp)
            e.setflags(write=False)
            self._expected[flags] = e
        self.expected = self._expected[flags]

    def chunk_byte(self, c):
        """The block offset of a byte inside chunk c."""
        p = int(np.searchsorted(self.pk["out_idx"], c, side="right")) - 1
        pk = self.pk[p]
        start = (c - int(pk["out_idx"])) * int(pk["bpc"])
        return int(pk["payload_off"]) + start + min(7, int(pk["len"]) - start - 1)

    def flip(self, chunks):
        """Flips one payload byte of every (block, chunk) given; calling it again restores them."""
        torch = _torch()
        if not chunks:
            return
        idx = torch.tensor([self.off[b] + self.chunk_byte(c) for b, c in chunks], dtype=torch.int64, device="cuda")
        assert idx.unique().numel() == len(chunks)
        self.t[idx] = self.t[idx] ^ 0x40


def _byte_order(sums, flags):
    """The stored form of host-order checksums (CRC32C_BIG_ENDIAN: byte-swapped)."""
    return sums.byteswap() if flags & mb.BE else sums


@pytest.fixture(scope="module")
def blockset(hdfs, gpu_ctx, orc):
    """The block set of a shape; one at a time is kept (the rows of a shape are adjacent in the table)."""
    held = {}

    def get(name):
        if name not in held:
            held.clear()
            held[name] = BlockSet(hdfs, gpu_ctx, orc, name)
        return held[name]

    return get


def _assert_report(case, plan, bs, nblocks, outs):
    """Both calls' launches as the row names them; no fall-back to one launch per block."""
    want = mb.launches_of(nblocks)
    assert len(want) == len(case.launches), case.id
    for verify in (False, True):
        got = plan.blocks_launch_info(bs.ptrs[:nblocks], None if verify else outs, verify)
        print("\n%s %s: %s" % (case.id, "verify" if verify else "exec", [
            (r.first_block, r.nblocks, r.ntiles, r.build.kernel, r.build.grid, r.general, r.skip_z, r.per_block)
            for r in got]))
        assert not any(r.per_block for r in got), (case.id, "falls back to one launch per block")
        assert [(r.first_block, r.nblocks) for r in got] == want, case.id
        for r, (kernel, skip_z, general) in zip(got, case.launches):
            t, w, m = mb.KERNELS[kernel]
            assert r.num_cu == bs.num_cu and r.ntiles == r.nblocks * bs.block_tiles, case.id
            assert r.build.kernel == (t, w, m | (mb.VERIFY if verify else 0)), \
                (case.id, r.first_block, "resize this row: the launch path now chooses", r.build.kernel, r.num_cu)
            assert (r.skip_z, r.general) == (skip_z, general), (case.id, r.first_block, r.skip_z, r.general)


@pytest.mark.parametrize("case", mb.CASES, ids=[c.id for c in mb.CASES])
def test_multi_block_row(hdfs, gpu_ctx, blockset, case):
    torch = _torch()
    bs = blockset(case.shape)
    nblocks = case.nblocks_at(bs.num_cu, bs.block_tiles)
    off = mb.misaligned_blocks(case.align, nblocks, bs.m)
    bs.place(off)
    bs.use_flags(case.flags)
    n = bs.n
    # plo is not block 0's address, and ONE_OFF's block is neither the first nor the lowest of its launch
    for first, count in mb.launches_of(nblocks):
        if count > 1:
            assert min(bs.ptrs[first:first + count]) != bs.ptrs[first]
    if case.align == mb.ONE_OFF:
        (b,) = off
        assert b != 0 and bs.ptrs[b] != min(bs.ptrs[:nblocks])
    plan = gpu_ctx.plan(bs.pk, case.flags)
    assert plan.nchecksums == n
    s = torch.cuda.Stream()
    try:
        # exec: one shared array, block b's checksums behind those of block b + 1, a guard word around each
        out = torch.full((nblocks * (n + 1) + 1,), OUT_FILL, dtype=torch.int32, device="cuda")
        at = [1 + (nblocks - 1 - b) * (n + 1) for b in range(nblocks)]
        outs = [out.data_ptr() + 4 * a for a in at]
        _assert_report(case, plan, bs, nblocks, outs)
        torch.cuda.synchronize()
        plan.exec_blocks(bs.ptrs[:nblocks], outs, s.cuda_stream)
        s.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        print("%s: %d blocks x %d checksums, %d bytes a block, %d off alignment; block 0 [0] got %08x want %08x" % (
            case.id, nblocks, n, bs.blen, len(off), got[at[0]], bs.expected[0][0]))
        for b in range(nblocks):
            diff = np.flatnonzero(got[at[b]:at[b] + n] != bs.expected[b])
            assert diff.size == 0, (case.id, "block %d: %d checksums differ, first %s" % (b, diff.size, diff[:8].tolist()))
        assert (got[0::n + 1] == OUT_FILL).all(), (case.id, "guard words written", np.flatnonzero(got[0::n + 1] != OUT_FILL))
        # verify: clean, then the corruption set
        run = Run(hdfs, plan, bs, nblocks)
        torch.cuda.synchronize()
        run.verify([], s.cuda_stream)
        run.check([], "%s, clean" % case.id)
        bad = corruption(n, nblocks)
        assert sum(p for _, _, p in bad) in (len(bad) // 2, (len(bad) + 1) // 2)  # half by payload, half by expectation
        run.verdicts.refill()
        run.work.refill()
        torch.cuda.synchronize()
        try:
            run.verify(bad, s.cuda_stream)
            run.check(bad, "%s, corrupted" % case.id)
        finally:
            run.unflip(bad)
    finally:
        torch.cuda.synchronize()
        plan.close()
