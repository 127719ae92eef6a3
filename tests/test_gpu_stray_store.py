"""No write-side kernel stores outside its checksums, no verify twin compares
or flags an index that is not its own.

Every other parity test reads back exactly the n words it expects, laid out
from index 0 without gaps: a store past either end lands in the allocator's
slack, and a store by a lane that should have been masked off lands on an
index another work item overwrites.  Here every output sits between guard
words (stray_store.GuardedWords, at all four word phases of a 16-byte
boundary), every packet's checksums are preceded by 64 uncovered words
(stray_store.gapped: a wave has 64 lanes), every launch runs over two fills,
and the WHOLE array -- guards and gaps included -- must read back as the
oracle's values on the covered indices and the fill everywhere else.

The verify twins get the same layouts: the expected values of gap and guard
words are ~fill, never a correct checksum of a neighbour, so a compare of a
lane that should not have compared counts a mismatch; the bitmap sits
between guards pre-filled with ones.

The partial-tile sweep (stray_store.FAMILIES / BANDS) runs every tile form at
every count of chunks a tile can hold, with every tail, aligned and 5 bytes
off, in every build select_plan_build can put it in; the last test of the
sweep checks that all eleven exec builds of cold_lds_cases.KERNELS and their
verify twins ran."""
from __future__ import annotations

import numpy as np
import pytest

import cold_lds_cases
import oracle
import stray_store as ss
from stray_store import GuardedWords, assert_image, expected_image, gapped

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _inv(fill: int) -> int:
    return ~fill & 0xFFFFFFFF


def _bits(words: np.ndarray) -> np.ndarray:
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little"))


def _bit_words(idx, nwords: int) -> np.ndarray:
    flags = np.zeros(32 * nwords, np.uint8)
    flags[np.asarray(idx, dtype=np.int64)] = 1
    return np.packbits(flags, bitorder="little").view("<u4")


class Device:
    """A host payload and its device copy; unchanged() reads the copy back."""

    def __init__(self, host: np.ndarray):
        torch = _torch()
        self.host = host
        self.host.setflags(write=False)
        self.t = torch.from_numpy(host.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr()

    def unchanged(self) -> bool:
        return bool(np.array_equal(self.t.cpu().numpy(), self.host))


def exec_both_fills(run, n: int, pk, want: np.ndarray, phase: int, what):
    """run(ptr) stores into a GuardedWords(n) at `phase`, once per fill (same plan
    and payload, the array refilled in between); the whole array must equal the
    expected image both times."""
    torch = _torch()
    out = GuardedWords(n, ss.FILLS[0], phase)
    for fill in ss.FILLS:
        out.refill(fill)
        torch.cuda.synchronize()
        run(out.ptr)
        torch.cuda.synchronize()
        assert_image(out.read(), expected_image(n, fill, pk, want, phase), "%s, fill %08x" % (what, fill))


def verify_steps(plan, payload_ptr: int, n: int, pk, want: np.ndarray, phase: int, stream, what):
    """verify and verify_bitmap over a clean expected array, then verify_bitmap
    with every third covered checksum and the last one flipped: results, bitmap
    and the bitmap's guards exact; expected values of gaps and guards are ~fill."""
    torch = _torch()
    words = -(-n // 32)
    cov = np.flatnonzero(ss.covered_mask(n, pk))
    bad = sorted(set(cov[::3].tolist()) | {int(cov[-1])})
    flipped = np.asarray(want, dtype=np.uint32).copy()
    flipped[bad] ^= np.uint32(1) << (np.asarray(bad, dtype=np.uint32) % np.uint32(32))
    exp = GuardedWords(n, 0, phase)
    res = GuardedWords(2, 0x77777777, (phase + 1) % 4)
    bits = GuardedWords(words, NONE, (phase + 2) % 4)
    for fill in ss.FILLS:
        # clean, without and with the bitmap
        exp.upload(expected_image(n, _inv(fill), pk, want, phase).words)
        for bitmap in (False, True):
            res.refill()
            bits.refill()
            torch.cuda.synchronize()
            plan.verify(payload_ptr, exp.ptr, res.ptr, stream.cuda_stream, dev_bad_bits=bits.ptr if bitmap else 0)
            stream.synchronize()
            assert_image(res.read(), expected_image(2, res.fill, None, np.array([0, NONE], np.uint32), res.phase),
                         "%s, clean result (bitmap %s, gaps %08x)" % (what, bitmap, _inv(fill)))
            want_bits = np.zeros(words, np.uint32) if bitmap else np.full(words, NONE, np.uint32)
            assert_image(bits.read(), expected_image(words, NONE, None, want_bits, bits.phase),
                         "%s, clean bitmap (bitmap %s)" % (what, bitmap))
        # mismatches: exactly the flipped set, no gap index
        exp.upload(expected_image(n, _inv(fill), pk, flipped, phase).words)
        res.refill()
        bits.refill()
        torch.cuda.synchronize()
        plan.verify(payload_ptr, exp.ptr, res.ptr, stream.cuda_stream, dev_bad_bits=bits.ptr)
        stream.synchronize()
        got = bits.read()
        set_bits = _bits(got[bits.lead:bits.lead + words])
        assert set_bits.tolist() == bad, "%s: bits %s set and should not be, %s clear and should be set" % (
            what, np.setdiff1d(set_bits, bad)[:8].tolist(), np.setdiff1d(bad, set_bits)[:8].tolist())
        assert_image(got, expected_image(words, NONE, None, _bit_words(bad, words), bits.phase), what + ", bitmap")
        assert_image(res.read(), expected_image(2, res.fill, None, np.array([len(bad), bad[0]], np.uint32), res.phase),
                     what + ", result of the flipped run")


def assert_build(plan, payload_ptr: int, kernel: str, what):
    t, w, m = cold_lds_cases.KERNELS[kernel]
    for verify in (False, True):
        info = plan.launch_info(payload_ptr, verify)
        assert info.build.kernel == (t, w, m | (cold_lds_cases.VERIFY if verify else 0)), \
            (what, "the launch path chooses", info.build.kernel, "at", info.num_cu, "CUs")


# ---- 1. the partial-tile sweep ---------------------------------------------------
_RAN = set()       # (kernel, verify) of every sweep case that ran to its end
_RAN_CASES = set()


@pytest.fixture(scope="module")
def num_cu(hdfs, gpu_ctx):
    plan = hdfs.Plan(gpu_ctx, oracle.uniform_packets(1))
    n = plan.launch_info(0).num_cu  # (the CU count launches are sized for)
    plan.close()
    return n


@pytest.fixture(scope="module")
def family_payload():
    """(family, off5) -> Device, made once: the family's packets and the ballast region behind them."""
    cache = {}

    def get(name, off5):
        if (name, off5) not in cache:
            pk = ss.with_ballast(name, ss.family_packets(name, off5), 1)
            cache[(name, off5)] = Device(oracle.xorshift64_bytes(ss.payload_bytes(pk, off5), 0x57A7 + len(cache)))
        return cache[(name, off5)]

    return get


@pytest.mark.parametrize("case", ss.SWEEP, ids=[c.id for c in ss.SWEEP])
def test_partial_tile_sweep(hdfs, gpu_ctx, orc, num_cu, family_payload, case):
    torch = _torch()
    s = torch.cuda.current_stream()
    dev = family_payload(case.family, case.off5)
    fam = ss.family_packets(case.family, case.off5)
    tiles, gen = hdfs.debug_plan(fam)
    pk = gapped(ss.with_ballast(case.family, fam, case.band.ballast(num_cu, tiles.size, gen.size)))
    off = ss.ptr_off(case.off5)
    assert int((pk["payload_off"] + pk["len"]).max()) + off + ss.SLACK <= dev.host.size
    n = hdfs.total_checksums(pk)
    want = orc.batch(dev.host[off:], pk, n)
    plan = hdfs.Plan(gpu_ctx, pk)
    assert plan.nchecksums == n
    try:
        assert_build(plan, dev.ptr + off, case.band.kernel, case.id)
        exec_both_fills(lambda out: plan.exec(dev.ptr + off, out, s.cuda_stream), n, pk, want, case.phase, case.id)
        verify_steps(plan, dev.ptr + off, n, pk, want, case.phase, s, case.id)
        assert dev.unchanged(), "%s: the payload was written" % case.id
    finally:
        torch.cuda.synchronize()
        plan.close()
    _RAN.update({(case.band.kernel, False), (case.band.kernel, True)})
    _RAN_CASES.add(case.id)


def test_sweep_ran_every_build():
    """Runs after the sweep: all eleven exec builds of cold_lds_cases.KERNELS and
    their verify twins ran it (each case asserted its build through launch_info
    before it ran).  It needs the whole sweep before it in the same session."""
    not_run = [c.id for c in ss.SWEEP if c.id not in _RAN_CASES]
    assert not not_run, "sweep cases that did not run to their end in this session: %s" % not_run
    missing = {(k, v) for k in cold_lds_cases.KERNELS for v in (False, True)} - _RAN
    assert not missing, "builds the sweep did not run: %s" % sorted(missing)


# ---- 2. the edges of verify_init ---------------------------------------------------
@pytest.mark.parametrize("words", [1, 2, 3, 4, 5, 7, 8, 9, 13])
def test_verify_init_bitmap_edges(hdfs, gpu_ctx, orc, words):
    """The bitmap is cleared with a scalar head, a uint4 body and a scalar tail:
    bad_words of 1..13 at all four word phases, pre-filled with ones, the first
    and the last checksum flipped -- exactly those two bits, both guards intact."""
    torch = _torch()
    s = torch.cuda.current_stream()
    n = 32 * words - 5
    pk = np.array([(0, 0, 512 * n, 512)], dtype=oracle.PACKET_DTYPE)
    dev = Device(oracle.xorshift64_bytes(512 * n + ss.SLACK, 0xED6E + words))
    want = orc.batch(dev.host, pk, n)
    flipped = want.copy()
    flipped[[0, n - 1]] ^= np.uint32(0x80000001)
    exp = torch.from_numpy(flipped.view(np.int32).copy()).cuda()
    plan = hdfs.Plan(gpu_ctx, pk)
    assert -(-plan.nchecksums // 32) == words
    try:
        for phase in range(4):
            bits = GuardedWords(words, NONE, phase)
            res = GuardedWords(2, 0x77777777, (phase + 1) % 4)
            torch.cuda.synchronize()
            plan.verify(dev.ptr, exp.data_ptr(), res.ptr, s.cuda_stream, dev_bad_bits=bits.ptr)
            s.synchronize()
            what = "bad_words %d, phase %d" % (words, phase)
            assert_image(bits.read(), expected_image(words, NONE, None, _bit_words([0, n - 1], words), phase), what)
            assert_image(res.read(), expected_image(2, res.fill, None, np.array([2, 0], np.uint32), res.phase), what)
    finally:
        torch.cuda.synchronize()
        plan.close()


# ---- 3. write plans (crc32c_plan_create_buffers) -----------------------------------
def _write_plan_case(hdfs, gpu_ctx, orc, bufs, stream_bytes, counts_want, phase, what):
    """A write plan at bpc 512 from block offset 0 (packets of 64 KiB: chunk i is
    bytes [512 i, 512 i + 512) of the assembled stream), exec and verify."""
    torch = _torch()
    s = torch.cuda.current_stream()
    counts = hdfs.debug_write_plan(bufs, 0, stream_bytes.size)
    for key, v in counts_want.items():
        assert counts[key] == v, (what, key, counts)
    want = orc.chunks(stream_bytes, 512)
    plan = gpu_ctx.write_plan(bufs, 0, stream_bytes.size, 0, 65536, 512)
    n = plan.nchecksums
    assert n == want.size == counts["nchecksums"]
    try:
        exec_both_fills(lambda out: plan.exec(0, out, s.cuda_stream), n, None, want, phase, what)
        verify_steps(plan, 0, n, None, want, phase, s, what)
    finally:
        torch.cuda.synchronize()
        plan.close()


@pytest.mark.parametrize("run", [1, 63, 64, 65, 1023, 1024, 1025])
def test_write_plan_constant_runs(hdfs, gpu_ctx, orc, run):
    """A zero-fill buffer last (the ftruncate extension) and a zero-fill buffer
    first, of `run` chunks: constant runs around the 64-lane loop's edge and
    kConstRunMax = 1024 (1025 chunks are two runs)."""
    data = Device(oracle.xorshift64_bytes(3 * 512 + 64, 0xC0 + run))
    head = (data.ptr + 16, 3 * 512)
    hb = data.host[16:16 + 3 * 512]
    zeros = np.zeros(512 * run, np.uint8)
    nruns = -(-run // 1024)
    _write_plan_case(hdfs, gpu_ctx, orc, [head, (0, zeros.size)], np.concatenate([hb, zeros]),
                     {"consts": nruns, "seg": 0, "gen": 0, "tiles": 1}, run % 4, "zero fill last, %d chunks" % run)
    # (1023 zero chunks first: the data's three chunks straddle a packet boundary, two tiles)
    _write_plan_case(hdfs, gpu_ctx, orc, [(0, zeros.size), head], np.concatenate([zeros, hb]),
                     {"consts": nruns, "seg": 0, "gen": 0, "tiles": 2 if run == 1023 else 1}, (run + 1) % 4,
                     "zero fill first, %d chunks" % run)
    assert data.unchanged()


def test_write_plan_spanning_chunk_at_the_end(hdfs, gpu_ctx, orc):
    """The plan's last chunk spans two buffers: a SegItem whose checksum is the
    very last word before the trailing guard."""
    a = Device(oracle.xorshift64_bytes(3 * 512 + 200 + 64, 0x5E61))
    b = Device(oracle.xorshift64_bytes(312 + 64, 0x5E62))
    for phase, (sa, sb) in enumerate(((0, 0), (16, 7), (3, 32), (9, 5))):
        bufs = [(a.ptr + sa, 3 * 512 + 200), (b.ptr + sb, 312)]
        stream_bytes = np.concatenate([a.host[sa:sa + 3 * 512 + 200], b.host[sb:sb + 312]])
        _write_plan_case(hdfs, gpu_ctx, orc, bufs, stream_bytes, {"seg": 1, "pieces": 2, "consts": 0, "nchecksums": 4},
                         phase, "spanning last chunk, skews %d / %d" % (sa, sb))
    assert a.unchanged() and b.unchanged()


# ---- 4. crc32c_plan_exec_blocks ---------------------------------------------------
NBLOCKS = 33  # two launches: 32 + 1


def _ragged_block(bpc: int) -> np.ndarray:
    """One block: 4 packets of 64 KiB, the last 300 bytes short, gapped."""
    pk = oracle.uniform_packets(4, bpc=bpc)
    pk["len"][-1] -= 300
    return gapped(ss.dense(pk))


@pytest.mark.parametrize("bpc", [512, 1024])
def test_exec_blocks_guarded(hdfs, gpu_ctx, orc, bpc):
    """33 blocks of a one-block, gapped, ragged shape, every third one off 16-byte
    alignment; every block's checksums in their own guarded array at phase
    b % 4, then all in one shared guarded array, 64 uncovered words between
    consecutive blocks.  At bpc 512 the short packet's 212-byte tail is a
    GenItem, and a plan with one runs one launch per block; at bpc 1024 the
    724-byte tail rides in a general tile and the 33 blocks run as two launches
    of 32 + 1 with per-block out_delta."""
    torch = _torch()
    s = torch.cuda.current_stream()
    pk = _ragged_block(bpc)
    n = hdfs.total_checksums(pk)
    tiles, gen = hdfs.debug_plan(pk)
    assert gen.size == (1 if bpc == 512 else 0), "the shape's launch form changed: see the docstring"
    blen = int((pk["payload_off"] + pk["len"]).max())
    slot = (blen + 15) // 16 * 16 + 64
    host = np.full(slot * NBLOCKS + ss.SLACK, 0xA5, np.uint8)
    stream_bytes = oracle.xorshift64_bytes(blen + 64 * NBLOCKS, 0xB10C + bpc)
    offs, wants = [], []
    for b in range(NBLOCKS):
        off = b * slot + 16 + (5 if b % 3 == 2 else 0)
        host[off:off + blen] = stream_bytes[64 * b:64 * b + blen]
        offs.append(off)
        wants.append(orc.batch(stream_bytes[64 * b:], pk, n))
    dev = Device(host)
    pays = [dev.ptr + o for o in offs]
    assert pays[2] % 16 == 5 and pays[0] % 16 == 0
    plan = gpu_ctx.plan(pk)
    assert plan.nchecksums == n
    try:
        outs = [GuardedWords(n, ss.FILLS[0], b % 4) for b in range(NBLOCKS)]
        for fill in ss.FILLS:
            for o in outs:
                o.refill(fill)
            torch.cuda.synchronize()
            plan.exec_blocks(pays, [o.ptr for o in outs], s.cuda_stream)
            torch.cuda.synchronize()
            for b, o in enumerate(outs):
                assert_image(o.read(), expected_image(n, fill, pk, wants[b], b % 4),
                             "bpc %d, block %d of %d, fill %08x" % (bpc, b, NBLOCKS, fill))
        # one shared array: block b's index 0 at word b (n + 64)
        step = n + ss.GAP
        total = step * NBLOCKS - ss.GAP
        allpk = np.concatenate([pk] * NBLOCKS)
        allpk["out_idx"] += np.repeat(np.arange(NBLOCKS, dtype=np.uint64) * np.uint64(step), pk.size)
        allwant = np.zeros(total, np.uint32)
        for b in range(NBLOCKS):
            allwant[b * step:b * step + n] = wants[b]
        shared = GuardedWords(total, ss.FILLS[0], 3)
        for fill in ss.FILLS:
            shared.refill(fill)
            torch.cuda.synchronize()
            plan.exec_blocks(pays, [shared.ptr + 4 * step * b for b in range(NBLOCKS)], s.cuda_stream)
            torch.cuda.synchronize()
            assert_image(shared.read(), expected_image(total, fill, allpk, allwant, 3),
                         "bpc %d, shared array, fill %08x" % (bpc, fill))
        assert dev.unchanged()
    finally:
        torch.cuda.synchronize()
        plan.close()


# ---- 5. the block queue, launch mode and resident mode ------------------------------
def _append_block(hdfs, length: int, blockoffset: int) -> np.ndarray:
    """One block write of `length` bytes at `blockoffset` as hadoop_rpc_send_packets
    cuts it (the first packet trimmed to a chunk boundary), packets back to back."""
    rows, off, oi = [], 0, 0
    for ln in hdfs.packetize(length, blockoffset, 65536, 512):
        if ln:
            rows.append((off, oi, ln, 512))
            off += ln
            oi += -(-ln // 512)
    return np.array(rows, dtype=oracle.PACKET_DTYPE)


@pytest.mark.parametrize("resident", [False, True], ids=["launch", "resident"])
def test_block_queue_guarded(hdfs, gpu_ctx, orc, resident):
    """16 blocks through submit / wait, half the aligned 4 MiB shape (the queue's
    plan), half an unaligned append with a GenItem at payload skews, every
    block's checksums gapped and in their own guarded array.  (Resident mode:
    the resident kernel's own store, which shares no code with the plan
    kernel's.  Outputs are filled before the first submit: a fill kernel waits
    for the resident kernel's idle exit.)"""
    torch = _torch()
    full = gapped(oracle.uniform_packets(64))
    append = gapped(_append_block(hdfs, 4 * 2**20 - 100, 100))
    assert hdfs.debug_plan(append)[1].size >= 1 and hdfs.debug_plan(full)[1].size == 0
    shapes = [full, append]
    ns = [hdfs.total_checksums(p) for p in shapes]
    host = oracle.xorshift64_bytes(4 * 2**20 + 64 * 16 + ss.SLACK, 0xB70C)
    dev = Device(host)
    jobs = []  # (shape index, payload byte offset)
    for k in range(16):
        jobs.append((k % 2, 64 * k + (0 if k % 2 == 0 else (k * 7) % 16)))
    assert all(off % 16 == 0 for si, off in jobs if si == 0) and any(off % 16 for si, off in jobs if si == 1)
    wants = [orc.batch(host[off:], shapes[si], ns[si]) for si, off in jobs]
    plans = [gpu_ctx.plan(p) for p in shapes]
    outs = [GuardedWords(ns[si], ss.FILLS[0], k % 4) for k, (si, _) in enumerate(jobs)]
    q = plans[0].blocks(resident=resident, idle_us=500, max_blocks=8, window_us=20)
    try:
        for fill in ss.FILLS:
            for o in outs:
                o.refill(fill)
            torch.cuda.synchronize()
            tickets = [q.submit(dev.ptr + off, outs[k].ptr, plan=plans[1] if si else None)
                       for k, (si, off) in enumerate(jobs)]
            q.flush()
            for t in tickets:
                q.wait(t)
            for k, (si, _) in enumerate(jobs):
                assert_image(outs[k].read(), expected_image(ns[si], fill, shapes[si], wants[k], k % 4),
                             "block %d (shape %d), fill %08x, resident %s" % (k, si, fill, resident))
        assert q.stats()[1] == 2 * len(jobs)
    finally:
        q.close()
        torch.cuda.synchronize()
        for p in plans:
            p.close()
    assert dev.unchanged()


# ---- 6. crc32c_batch_host ------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_batch_host_guarded(hdfs, gpu_ctx, orc, pinned):
    """A gapped batch into a host array pre-filled with each fill (the host path
    scatters per packet): the whole array, guards included."""
    torch = _torch()
    pk = gapped(np.concatenate([ss.family_packets("pow2"), ss.family_packets("general")[:40]]))
    pk["payload_off"][-40:] += np.uint64(1 << 20)  # (the second family's packets behind the first's)
    n = hdfs.total_checksums(pk)
    size = (int((pk["payload_off"] + pk["len"]).max()) + ss.SLACK + 15) // 16 * 16
    payload = oracle.xorshift64_bytes(size, 0x4057)
    want = orc.batch(payload, pk, n)
    src = torch.from_numpy(payload.copy()).pin_memory().numpy() if pinned else payload.copy()
    for phase, fill in enumerate(ss.FILLS):
        lead, total = ss.layout(n, phase + 1)
        arr = np.full(total, fill, np.uint32)
        got = gpu_ctx.batch_host(src, pk, out=arr[lead:lead + n])
        assert got.ctypes.data == arr.ctypes.data + 4 * lead
        assert_image(arr, expected_image(n, fill, pk, want, phase + 1), "batch_host, fill %08x" % fill)
    assert np.array_equal(src, payload)


# ---- 7. the multi-GPU plan's packed gather on one GPU ----------------------------------
def test_multi_plan_packed_gather_guarded(hdfs, orc):
    """The shape of test_multi_plan_self_send_several_transfers_per_peer (12 groups
    whose checksum ranges leave gaps of 37 words), packed: one send / receive
    pair to self into the staging array, then the scatter kernel's stores into
    file order -- root_out between guards at phase 1, both fills."""
    torch = _torch()
    gp, ngroups, gap = 3, 12, 37
    pk = oracle.uniform_packets(gp * ngroups)
    per = 128 * gp
    pk["out_idx"] = np.array([(i // gp) * (per + gap) + (i % gp) * 128 for i in range(pk.size)], np.uint64)
    payload = oracle.xorshift64_bytes(int((pk["payload_off"] + pk["len"]).max()) + 16, 515)
    total = int((pk["out_idx"] + 128).max())
    want = orc.batch(payload, pk, total)
    m = hdfs.Multi([0])
    mp = m.plan(pk, gp, hdfs.CRC32C_MULTI_SELF_SEND)
    try:
        assert mp.nchecksums == total and mp.gather_ops() == (2, True)
        layout, sb = hdfs.multi_layout(pk, gp, 1)
        host = np.zeros(int(sb[0]) + 16, np.uint8)
        for _, soff, poff, nbytes in layout.astype(np.int64):
            host[soff:soff + nbytes] = payload[poff:poff + nbytes]
        shard = Device(host)
        out = GuardedWords(total, ss.FILLS[0], 1)
        for fill in ss.FILLS:
            out.refill(fill)
            torch.cuda.synchronize()
            mp.exec([shard.ptr], out.ptr)
            m.sync()
            torch.cuda.synchronize()
            assert_image(out.read(), expected_image(total, fill, pk, want, 1), "packed gather, fill %08x" % fill)
        assert shard.unchanged()
    finally:
        mp.close()
        m.close()
