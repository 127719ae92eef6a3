"""Many blocks verified in one call (include/hdfs_crc32c.h sections 3c and 6d;
csrc/crc32c_verdicts.hip, crc32c_plan_verify_blocks in csrc/crc32c_runtime.hip).

crc32c_bitmap_verdicts is compared with its host twin (itself checked against
numpy in tests/test_verdicts_host.py, whose size and pattern tables are used
here) at sizes placed from the kernel's geometry hook.  crc32c_plan_verify_blocks
is compared with verdicts worked out from the set of corrupted chunks; the
expected checksums come from the oracle (zlib for CRC32C_TYPE_CRC32), none of
this library's code is in them.  Every device buffer the calls write sits
between guard bytes that must come back unchanged, every bitmap they read is
followed by words of ones."""
from __future__ import annotations

import ctypes
import errno

import numpy as np
import pytest

import oracle
from test_verdicts_host import CELL_SIZES, NONE, PATTERNS, as_rows, make_bits, nsums_table, pack

pytestmark = pytest.mark.gpu

BE = 0x1     # CRC32C_BIG_ENDIAN
CRC32 = 0x2  # CRC32C_TYPE_CRC32
GUARD_BYTES = 64


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X (cuda:0)"
    return torch


class Guarded:
    """nbytes of device memory filled with `fill`, `phase` bytes past a 16-byte
    boundary, between two runs of guard bytes of the same fill."""

    def __init__(self, nbytes: int, fill: int, phase: int = 4):
        torch = _torch()
        self.nbytes, self.fill, self.lead = nbytes, fill, GUARD_BYTES + phase
        self.t = torch.full((nbytes + 2 * GUARD_BYTES + 16,), fill, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lead

    def refill(self):
        self.t.fill_(self.fill)

    def put(self, data: np.ndarray, byte_off: int = 0):
        torch = _torch()
        b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert byte_off + b.size <= self.nbytes
        if b.size:
            self.t[self.lead + byte_off:self.lead + byte_off + b.size] = torch.from_numpy(b.copy()).cuda()

    def read(self) -> np.ndarray:
        """The bytes (a copy); asserts both guards intact."""
        _torch().cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:self.lead] == self.fill).all(), "bytes before the buffer were written"
        assert (h[self.lead + self.nbytes:] == self.fill).all(), "bytes after the buffer were written"
        return h[self.lead:self.lead + self.nbytes].copy()

    def untouched(self) -> bool:
        _torch().cuda.synchronize()
        return bool((self.t.cpu().numpy() == self.fill).all())


@pytest.fixture(scope="module")
def geom(hdfs):
    return hdfs.debug_verdict_geometry()


# ---- 1. crc32c_bitmap_verdicts against the host twin --------------------------
def _device_verdicts(hdfs, gpu_ctx, words, nsums, cpc, stream=0):
    """The device call over the bitmap 4 bytes past a 16-byte boundary and
    followed by ones; the verdict rows, read from between guards."""
    ncells = hdfs.md5_nblocks(nsums, cpc)
    bits = Guarded(4 * words.size, 0xFF, phase=4)
    bits.put(words)
    out = Guarded(16 * ncells, 0xEE, phase=4)
    gpu_ctx.bitmap_verdicts(bits.ptr, nsums, cpc, out.ptr, stream)
    return as_rows(out.read().view(hdfs.BLOCK_VERDICT_DTYPE))


def _check_rows(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: cells %s differ (first: got %s, want %s)" % (
        what, bad[:8].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


def _cell_sizes(geom):
    m = geom["lane_max_cell"]
    return sorted(set(CELL_SIZES + [m - 1, m, m + 1]))


def test_verdict_cell_sizes_cover_both_forms(geom):
    sizes = _cell_sizes(geom)
    assert min(sizes) <= geom["lane_max_cell"] < max(sizes)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_bitmap_verdicts_against_host_twin(hdfs, gpu_ctx, geom, pattern):
    cells = 0
    for cpc in _cell_sizes(geom):
        for nsums in nsums_table(cpc):
            words = pack(make_bits(pattern, nsums, cpc, seed=1))
            want = as_rows(hdfs.bitmap_verdicts_host(words, nsums, cpc))
            got = _device_verdicts(hdfs, gpu_ctx, words, nsums, cpc)
            _check_rows(got, want, "cpc %d, nsums %d, %s" % (cpc, nsums, pattern))
            cells += want.shape[0]
    assert cells >= 10 * len(CELL_SIZES)


def test_bitmap_verdicts_past_the_grid_cap(hdfs, gpu_ctx, geom):
    """More cells than a capped grid has lanes (lane form) or waves (wave form):
    the launch strides over them."""
    per_wg = geom["lanes"] * geom["waves_per_workgroup"]
    big = geom["lane_max_cell"] + 1
    for cpc, ncells in ((1, geom["grid_cap"] * per_wg + 3), (3, geom["grid_cap"] * per_wg + 1),
                        (big, geom["grid_cap"] * geom["waves_per_workgroup"] + 2)):
        nsums = (ncells - 1) * cpc + 1
        words = pack(make_bits("half", nsums, cpc, seed=2))
        want = as_rows(hdfs.bitmap_verdicts_host(words, nsums, cpc))
        assert want.shape[0] == ncells
        _check_rows(_device_verdicts(hdfs, gpu_ctx, words, nsums, cpc), want, "cpc %d, %d cells" % (cpc, ncells))


def test_bitmap_verdicts_graph_replayed_twice(hdfs, gpu_ctx, geom):
    """One captured call of each form, replayed twice over a bitmap changed in
    between: nothing is accumulated, every verdict is rewritten."""
    torch = _torch()
    cases = [(geom["lane_max_cell"], 37 * geom["lane_max_cell"] + 5), (2049, 9 * 2049 + 11)]
    bufs = [(Guarded(4 * (-(-nsums // 32)), 0xFF, phase=4), Guarded(16 * hdfs.md5_nblocks(nsums, cpc), 0xEE, phase=4))
            for cpc, nsums in cases]
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        for (cpc, nsums), (bits, out) in zip(cases, bufs):
            gpu_ctx.bitmap_verdicts(bits.ptr, nsums, cpc, out.ptr, cap.cuda_stream)
    torch.cuda.synchronize()
    assert all(out.untouched() for _, out in bufs), "the capture itself ran the kernel"
    for r, pattern in enumerate(("half", "sparse")):
        for (cpc, nsums), (bits, out) in zip(cases, bufs):
            bits.put(pack(make_bits(pattern, nsums, cpc, seed=10 + r)))
        torch.cuda.synchronize()
        g.replay()
        for (cpc, nsums), (bits, out) in zip(cases, bufs):
            words = pack(make_bits(pattern, nsums, cpc, seed=10 + r))
            _check_rows(as_rows(out.read().view(hdfs.BLOCK_VERDICT_DTYPE)),
                        as_rows(hdfs.bitmap_verdicts_host(words, nsums, cpc)), "replay %d, cpc %d" % (r, cpc))
    del g


def test_bitmap_verdicts_rejections(hdfs, gpu_ctx):
    bits = Guarded(64, 0xFF)
    out = Guarded(16 * 8, 0x77)
    closed = hdfs.Context.__new__(hdfs.Context)
    closed.handle, closed.device = None, 0
    refused = [
        ("NULL ctx", lambda: closed.bitmap_verdicts(bits.ptr, 64, 16, out.ptr)),
        ("crc_per_cell 0", lambda: gpu_ctx.bitmap_verdicts(bits.ptr, 64, 0, out.ptr)),
        ("NULL bitmap", lambda: gpu_ctx.bitmap_verdicts(0, 64, 16, out.ptr)),
        ("NULL verdicts", lambda: gpu_ctx.bitmap_verdicts(bits.ptr, 64, 16, 0)),
        ("bitmap off 4-byte alignment", lambda: gpu_ctx.bitmap_verdicts(bits.ptr + 2, 64, 16, out.ptr)),
        ("verdicts off 4-byte alignment", lambda: gpu_ctx.bitmap_verdicts(bits.ptr, 64, 16, out.ptr + 1)),
    ]
    for what, call in refused:
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == -errno.EINVAL, what
    gpu_ctx.bitmap_verdicts(0, 0, 16, 0)
    gpu_ctx.bitmap_verdicts(bits.ptr, 0, 0, out.ptr)
    assert out.untouched() and bits.untouched()


# ---- 2. crc32c_plan_verify_blocks ----------------------------------------------
MAX_BLOCKS = 65
BLOCK_COUNTS = (1, 2, 32, 33, 65)


def _packets(hdfs, lens, bpc):
    rows, pos, idx = [], 0, 0
    for plen in lens:
        rows.append((pos, idx, plen, bpc))
        pos += plen
        idx += -(-plen // bpc)
    return np.array(rows, dtype=hdfs.PACKET_DTYPE), pos, idx


# name: (packet lengths, bpc, flags)
# (b): n = 258 = 2 mod 32, so blocks share bitmap words, and the last packet's
# 976-byte tail chunk rides in a general tile.  (Packets of 65536, 65536 and
# 1000 bytes at bpc 512 also give n = 258, but their 488-byte tail is a work
# item of its own, not a tile -- plan.cpp sends a tail of at most one 512-byte
# block behind power-of-two chunks there -- so that plan has no multi-block
# form: test_verify_blocks_rejections checks that it is refused.)
SHAPES = {
    "a": ([65536] * 16, 512, 0),             # n = 2048
    "b": ([131072, 133072], 1024, 0),        # n = 258: a general tail tile
    "c": ([98304, 98304, 5000], 1536, 0),    # n = 132: general tiles
    "d": ([65536] * 16, 512, BE),
    "e": ([65536] * 16, 512, CRC32),
}


class BlockSet:
    """MAX_BLOCKS distinct blocks of one shape in device memory, in shuffled
    slots, every third one 5 bytes off 16-byte alignment, and their expected
    checksums in the plan's stored order (from the oracle / zlib)."""

    def __init__(self, hdfs, orc, name):
        torch = _torch()
        lens, self.bpc, self.flags = SHAPES[name]
        self.pk, self.blen, self.n = _packets(hdfs, lens, self.bpc)
        stream = oracle.xorshift64_bytes(self.blen + 64 * MAX_BLOCKS, 0x5EED0 + ord(name))
        slot = (self.blen + 15) // 16 * 16 + 32
        perm = np.random.default_rng(ord(name)).permutation(MAX_BLOCKS)
        self.t = torch.full((slot * MAX_BLOCKS + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.off, exp = [], []
        for b in range(MAX_BLOCKS):
            data = stream[64 * b:64 * b + self.blen]
            off = int(perm[b]) * slot + 16 + (5 if b % 3 == 2 else 0)
            self.t[off:off + self.blen] = torch.from_numpy(data.copy()).cuda()
            self.off.append(off)
            if self.flags & CRC32:
                exp.append(oracle.zlib_batch(data, self.pk, self.n))
            else:
                exp.append(orc.batch(data, self.pk, self.n, big_endian=bool(self.flags & BE)))
        self.expected = np.stack(exp)
        self.expected.setflags(write=False)
        self.ptrs = [self.t.data_ptr() + o for o in self.off]
        assert any(self.ptrs[i + 1] < self.ptrs[i] for i in range(MAX_BLOCKS - 1))  # non-monotonic
        assert self.ptrs[2] % 16 == 5 and self.ptrs[0] % 16 == 0

    def flip(self, chunks):
        """Flips one payload byte of every (block, chunk) given (every shape here:
        chunk c of a block starts at byte c * bpc); calling it again restores them."""
        torch = _torch()
        if not chunks:
            return
        idx = torch.tensor([self.off[b] + c * self.bpc + min(7, self.blen - c * self.bpc - 1) for b, c in chunks],
                           dtype=torch.int64, device="cuda")
        self.t[idx] = self.t[idx] ^ 0x40


@pytest.fixture(scope="module")
def blocksets(hdfs, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = BlockSet(hdfs, orc, name)
        return cache[name]

    return get


def corruption(n: int, nblocks: int):
    """[(block, chunk, by_payload)]: chunk 0 of block 0; the last chunk of the
    last block; the last chunk of a block and the first of the next (blocks 0
    and 1: a shared bitmap word when n % 32 != 0); the launch seam (blocks 31 and
    32); one block with every chunk bad.  Half by a payload byte, half by an
    expected word."""
    c = {(0, 0): True, (nblocks - 1, n - 1): False}
    if nblocks >= 2:
        c.setdefault((0, n - 1), False)
        c.setdefault((1, 0), True)
    if nblocks >= 33:
        c.setdefault((31, n - 1), True)
        c.setdefault((32, 0), False)
    if nblocks >= 3:
        full = nblocks // 2
        for k in range(n):
            c.setdefault((full, k), k % 2 == 0)
    return [(b, k, p) for (b, k), p in sorted(c.items())]


def expected_outcome(bad, n, nblocks):
    """Verdict rows, the bitmap's words and the per-launch results of a set of bad (block, chunk)."""
    bits = np.zeros(nblocks * n, np.uint8)
    for b, k, _ in bad:
        bits[b * n + k] = 1
    rows = np.zeros((nblocks, 4), np.uint32)
    for b in range(nblocks):
        nz = np.flatnonzero(bits[b * n:(b + 1) * n])
        rows[b] = (nz.size, nz[0] if nz.size else NONE, nz[-1] if nz.size else NONE, 0)
    padded = np.zeros(-(-bits.size // 32) * 32, np.uint8)
    padded[:bits.size] = bits
    words = np.packbits(padded, bitorder="little").view("<u4")
    results = []
    for g in range(-(-nblocks // 32)):
        nz = np.flatnonzero(bits[32 * g * n:32 * (g + 1) * n])
        results += [nz.size, nz[0] if nz.size else NONE]
    return rows, words, np.array(results, np.uint32)


class Run:
    """Device buffers of one verify_blocks call: expected values inside a filled
    buffer, verdicts and work area between guards, all pre-filled with 0xFF."""

    def __init__(self, hdfs, plan, bs, nblocks):
        self.hdfs, self.plan, self.bs, self.nblocks = hdfs, plan, bs, nblocks
        self.exp = Guarded(4 * bs.n * nblocks, 0xA5, phase=4)
        self.verdicts = Guarded(16 * nblocks, 0xFF, phase=4)
        self.work_bytes = plan.verify_blocks_work_bytes(nblocks)
        self.bitmap_words = -(-nblocks * bs.n // 32)
        assert self.work_bytes == 4 * (self.bitmap_words + 2 * -(-nblocks // 32))
        self.work = Guarded(self.work_bytes, 0xFF, phase=4)

    def verify(self, bad, stream=0, launch=True):
        """Uploads the expected values with `bad`'s expected-word flips and makes the
        payload flips; launch=False: only that.  Undo the payload flips with unflip()."""
        exp = self.bs.expected[:self.nblocks].copy()
        for b, k, by_payload in bad:
            if not by_payload:
                exp[b, k] ^= 0x00010000
        self.bs.flip([(b, k) for b, k, by_payload in bad if by_payload])
        self.exp.put(exp)
        _torch().cuda.synchronize()  # (the uploads ran on torch's stream)
        if launch:
            self.plan.verify_blocks(self.bs.ptrs[:self.nblocks], self.exp.ptr, self.verdicts.ptr, self.work.ptr, stream)

    def unflip(self, bad):
        _torch().cuda.synchronize()
        self.bs.flip([(b, k) for b, k, by_payload in bad if by_payload])

    def check(self, bad, what):
        rows, words, results = expected_outcome(bad, self.bs.n, self.nblocks)
        got = as_rows(self.verdicts.read().view(self.hdfs.BLOCK_VERDICT_DTYPE))
        _check_rows(got, rows, what)  # (exact: bit 31 is clear everywhere)
        work = self.work.read().view(np.uint32)
        assert (work[:self.bitmap_words] == words).all(), "%s: bitmap words %s differ" % (
            what, np.flatnonzero(work[:self.bitmap_words] != words)[:8].tolist())
        assert (work[self.bitmap_words:] == results).all(), "%s: launch results %s, want %s" % (
            what, work[self.bitmap_words:].tolist(), results.tolist())
        clean = np.setdiff1d(np.arange(self.nblocks), [b for b, _, _ in bad])
        assert (got[clean] == np.array([0, NONE, NONE, 0], np.uint32)).all(), what


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_verify_blocks_clean_and_corrupted(hdfs, gpu_ctx, blocksets, shape):
    torch = _torch()
    bs = blocksets(shape)
    plan = gpu_ctx.plan(bs.pk, bs.flags)
    assert plan.nchecksums == bs.n
    s = torch.cuda.Stream()
    try:
        for nblocks in BLOCK_COUNTS:
            run = Run(hdfs, plan, bs, nblocks)
            torch.cuda.synchronize()
            run.verify([], s.cuda_stream)
            run.check([], "shape %s, %d blocks, clean" % (shape, nblocks))
            bad = corruption(bs.n, nblocks)
            run.verdicts.refill()
            run.work.refill()
            torch.cuda.synchronize()
            try:
                run.verify(bad, s.cuda_stream)
                run.check(bad, "shape %s, %d blocks, corrupted" % (shape, nblocks))
                if shape == "a" and nblocks == 33:
                    _compare_with_per_block_verify(hdfs, plan, run, s)
            finally:
                run.unflip(bad)
    finally:
        torch.cuda.synchronize()
        plan.close()


def _compare_with_per_block_verify(hdfs, plan, run, s):
    """crc32c_plan_verify_bitmap once per block over the same (corrupted) data:
    the same count, first index and bits as the one call's verdicts and bitmap."""
    n, nblocks = run.bs.n, run.nblocks
    got = as_rows(run.verdicts.read().view(hdfs.BLOCK_VERDICT_DTYPE))
    bits = np.unpackbits(run.work.read()[:4 * run.bitmap_words], bitorder="little")[:nblocks * n]
    res = Guarded(8 * nblocks, 0xEE, phase=0)
    bm = Guarded(4 * (-(-n // 32)) * nblocks, 0xEE, phase=0)
    _torch().cuda.synchronize()
    for b in range(nblocks):
        plan.verify(run.bs.ptrs[b], run.exp.ptr + 4 * n * b, res.ptr + 8 * b, s.cuda_stream,
                    dev_bad_bits=bm.ptr + 4 * (-(-n // 32)) * b)
    r = res.read().view(np.uint32).reshape(nblocks, 2)
    assert (r[:, 0] == got[:, 0]).all() and (r[:, 1] == got[:, 1]).all()
    per = np.unpackbits(bm.read(), bitorder="little").reshape(nblocks, -1)[:, :n]
    assert (per.reshape(-1) == bits).all()


# ---- 3. stale scratch ---------------------------------------------------------------
@pytest.mark.parametrize("shape", ["a", "b"])
def test_stale_scratch_and_graph_replay(hdfs, gpu_ctx, blocksets, shape):
    """dev_work and dev_verdicts start as 0xFF.  A corrupted run and then a clean
    one on the same buffers: every verdict clean, the bitmap zero.  Then the call
    captured over clean data and replayed once over data corrupted after the
    capture: the replay reports the corruption."""
    torch = _torch()
    bs = blocksets(shape)
    nblocks = 33
    plan = gpu_ctx.plan(bs.pk, bs.flags)
    cap = torch.cuda.Stream()
    run = Run(hdfs, plan, bs, nblocks)
    bad = corruption(bs.n, nblocks)
    torch.cuda.synchronize()
    try:
        run.verify(bad, cap.cuda_stream)
    finally:
        run.unflip(bad)
    run.check(bad, "corrupted run")
    run.verify([], cap.cuda_stream)
    run.check([], "clean run over the corrupted run's buffers")
    plan.close()
    # a fresh plan, so that its first verify launch is the captured one
    plan = gpu_ctx.plan(bs.pk, bs.flags)
    run = Run(hdfs, plan, bs, nblocks)
    run.verify([], launch=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        plan.verify_blocks(bs.ptrs[:nblocks], run.exp.ptr, run.verdicts.ptr, run.work.ptr, cap.cuda_stream)
    torch.cuda.synchronize()
    assert run.verdicts.untouched() and run.work.untouched(), "the capture itself ran the kernels"
    try:
        run.verify(bad, launch=False)
        torch.cuda.synchronize()
        g.replay()
        run.check(bad, "replay over data corrupted after the capture")
    finally:
        run.unflip(bad)
    del g
    plan.close()


# ---- 4. rejections -------------------------------------------------------------------
def test_verify_blocks_rejections(hdfs, gpu_ctx, blocksets):
    """Every refused call returns -EINVAL and leaves dev_verdicts and dev_work
    with their fill; nblocks == 0 returns 0 and leaves it too."""
    torch = _torch()
    bs = blocksets("b")
    plan = gpu_ctx.plan(bs.pk, bs.flags)
    run = Run(hdfs, plan, bs, 2)
    run.verify([], launch=False)
    p2, e, v, w = bs.ptrs[:2], run.exp.ptr, run.verdicts.ptr, run.work.ptr
    tail3, _, _ = _packets(hdfs, [65536 + 3], 512)  # a 3-byte packet tail: a general item, not a tile
    gen_plan = gpu_ctx.plan(tail3, 0)
    tail488, _, n488 = _packets(hdfs, [65536, 65536, 1000], 512)  # a 488-byte tail behind bpc-512 chunks: the same
    assert n488 == 258
    tail_plan = gpu_ctx.plan(tail488, 0)
    abs_pk = bs.pk.copy()
    abs_pk["payload_off"] += bs.ptrs[0]
    abs_plan = gpu_ctx.plan(abs_pk, hdfs.CRC32C_DEVICE_ADDRESSES)
    buf_plan = gpu_ctx.write_plan([(bs.ptrs[0], bs.blen)], 0, bs.blen)
    L, vp = hdfs.lib(), ctypes.c_void_p
    refused = [
        ("a non-tile plan", lambda: gen_plan.verify_blocks(p2, e, v, w)),
        ("a non-tile plan (a 488-byte tail at bpc 512)", lambda: tail_plan.verify_blocks(p2, e, v, w)),
        ("a device-address plan", lambda: abs_plan.verify_blocks(p2, e, v, w)),
        ("a buffer-list plan", lambda: buf_plan.verify_blocks(p2, e, v, w)),
        ("NULL payload", lambda: plan.verify_blocks([p2[0], 0], e, v, w)),
        ("NULL expected", lambda: plan.verify_blocks(p2, 0, v, w)),
        ("NULL verdicts", lambda: plan.verify_blocks(p2, e, 0, w)),
        ("NULL work", lambda: plan.verify_blocks(p2, e, v, 0)),
        ("expected off 4-byte alignment", lambda: plan.verify_blocks(p2, e + 2, v, w)),
        ("verdicts off 4-byte alignment", lambda: plan.verify_blocks(p2, e, v + 1, w)),
        ("work off 4-byte alignment", lambda: plan.verify_blocks(p2, e, v, w + 3)),
    ]
    for what, call in refused:
        with pytest.raises(hdfs.Crc32cError) as err:
            call()
        assert err.value.rc == -errno.EINVAL, what
    assert L.crc32c_plan_verify_blocks(plan.handle, None, vp(e), 2, vp(v), vp(w), None) == -errno.EINVAL
    assert L.crc32c_plan_verify_blocks(None, None, vp(e), 2, vp(v), vp(w), None) == -errno.EINVAL
    plan.verify_blocks([], e, v, w)
    assert plan.verify_blocks_work_bytes(0) == 0
    torch.cuda.synchronize()
    assert run.verdicts.untouched() and run.work.untouched()
    # the plan still verifies after the refusals
    run.verify([])
    run.check([], "after the refusals")
    for p in (plan, gen_plan, tail_plan, abs_plan, buf_plan):
        p.close()
