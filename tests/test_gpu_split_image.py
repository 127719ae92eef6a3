"""Every build that stages the split S4 image, against the oracle.

The full-image production builds (bulk, the three general builds, the two
half-tile builds, each exec and verify) and the resident kernel look their
byte tables up in the split image: 16 columns per table, lanes 0-15 of a
half-wave reading one table of a pair while lanes 16-31 read the other
(csrc/crc32c_device.h s4<kImgSplit>).  Each case here is the smallest batch
that still selects its build (more than kSmallBatchItemsPerCu work items per
CU), asserted through crc32c_debug_select_build, over one payload of two
parts: PCG random bytes, and in front of them a one-hot region of 512-byte
blocks that are zero but for one byte -- every value 1..255 at every byte
offset 0..15 of a lane's piece, in a piece of each lane half (columns 3 and
19): every table row through both lane roles and every position of the
lookup chain.  Exec must equal the oracle bit for bit; verify must report 0
mismatches on the right checksums and the flipped index with one flipped.
(The resident queue stores only: it has no comparing form.)"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import pytest

import cold_lds_cases
import oracle
from cold_lds_cases import Shape

pytestmark = pytest.mark.gpu

ONE_HOT_COLUMNS = (3, 19)
ONE_HOT_BLOCKS = 255 * 16 * len(ONE_HOT_COLUMNS)  # 8160
PAYLOAD_BYTES = 521 * 65536 + 8192


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def one_hot_region() -> np.ndarray:
    blocks = np.zeros((ONE_HOT_BLOCKS, 512), np.uint8)
    i = 0
    for q in ONE_HOT_COLUMNS:
        for k in range(16):
            for val in range(1, 256):
                blocks[i, 16 * q + k] = val
                i += 1
    assert i == ONE_HOT_BLOCKS
    return blocks.reshape(-1)


@pytest.fixture(scope="module")
def payload():
    torch = _torch()
    host = np.random.Generator(np.random.PCG64(0x5917)).integers(0, 256, PAYLOAD_BYTES, dtype=np.uint8)
    hot = one_hot_region()
    host[:hot.size] = hot
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    return host, dev


class Case(NamedTuple):
    id: str
    shape: Shape
    per_cu8: int   # packets = per_cu8 * CUs / 8 + 8
    kernel: str    # cold_lds_cases.KERNELS key
    skip_z: int
    general: int
    crc32: bool = False


CASES = [
    Case("bpc512-bulk", Shape(512), 16, "bulk", 1, 0),
    Case("bpc1024-bulk-z", Shape(1024), 16, "bulk", 0, 0),
    Case("bpc8192-bulk-z", Shape(8192), 16, "bulk", 0, 0),
    Case("bpc1000-both-paths", Shape(1000, first=64), 16, "both_hoist", 0, 11),
    # one general tile per packet: 3 chunks of 1536 bytes and a 412-byte tail
    Case("tail412-general-tiles-only", Shape(1536, pkt_len=3 * 1536 + 412, stride=5024), 128, "gitems", 0, 1),
    Case("off5-shifted-only", Shape(512, first=5), 16, "shift", 1, 2),
    Case("bpc700-half-aligned", Shape(700, pkt_len=65100, first=64), 16, "half", 0, 5),
    Case("bpc700-half-unaligned", Shape(700, pkt_len=65100, first=64, ptr_off=5), 16, "half_shift", 0, 7),
    Case("bpc512-bulk-crc32", Shape(512), 16, "bulk", 1, 0, crc32=True),
]


def _assert_build(hdfs, plan, dev_payload, case):
    t, w, m = cold_lds_cases.KERNELS[case.kernel]
    for verify in (False, True):
        info = plan.launch_info(dev_payload, verify)
        want = (t, w, m | (cold_lds_cases.VERIFY if verify else 0))
        picked = hdfs.debug_select_build(info.ntiles, info.ngen, info.nseg, info.nconst, info.general, verify,
                                         info.num_cu)
        assert picked.kernel == want and info.build.kernel == want, (case.id, picked.kernel, info.build.kernel)
        assert (info.skip_z, info.general) == (case.skip_z, case.general), (case.id, info.skip_z, info.general)
        items = info.ntiles + (info.ngen + 1) // 2
        assert items > 16 * info.num_cu, (case.id, items)  # (no small-batch build)


def _verify(plan, dev_payload, expected, stream):
    torch = _torch()
    res = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dev_exp = torch.from_numpy(expected.view(np.int32).copy()).cuda()
    plan.verify(dev_payload, dev_exp.data_ptr(), res.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return res.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_split_image_build(hdfs, gpu_ctx, orc, payload, case):
    torch = _torch()
    host, dev = payload
    s = torch.cuda.current_stream()
    plan0 = hdfs.Plan(gpu_ctx, oracle.uniform_packets(1))
    num_cu = plan0.launch_info(dev.data_ptr()).num_cu
    plan0.close()
    shape = case.shape
    pk = cold_lds_cases.packets(shape, case.per_cu8 * num_cu // 8 + 8)
    assert int((pk["payload_off"] + pk["len"]).max()) + shape.ptr_off + 4096 <= host.size
    n = hdfs.total_checksums(pk)
    flags = hdfs.CRC32C_TYPE_CRC32 if case.crc32 else 0
    if case.crc32:
        want = oracle.zlib_batch(host[shape.ptr_off:], pk, n)
    else:
        want = orc.batch(host[shape.ptr_off:], pk, n)
    plan = hdfs.Plan(gpu_ctx, pk, flags)
    dev_payload = dev.data_ptr() + shape.ptr_off
    _assert_build(hdfs, plan, dev_payload, case)
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    plan.exec(dev_payload, out.data_ptr(), s.cuda_stream)
    s.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), (case.id, np.flatnonzero(got != want)[:8])
    assert _verify(plan, dev_payload, want, s) == [0, 0xFFFFFFFF], case.id
    for k in (0, n // 2 + 1, n - 1):
        flipped = want.copy()
        flipped[k] ^= np.uint32(1 << (k % 32))
        assert _verify(plan, dev_payload, flipped, s) == [1, k], (case.id, k)
    plan.close()


def test_32_column_variant_is_still_exact(hdfs, gpu_ctx, orc, payload):
    """The debug library keeps the 32-column image as variants of the bulk
    build (97; 98 stamped; 99 the split image stamped), so that old and new
    can be timed in one process: all three still compute the oracle's values."""
    torch = _torch()
    host, dev = payload
    s = torch.cuda.current_stream()
    pk = oracle.uniform_packets(64)  # (covers the one-hot region)
    assert 64 * 65536 >= ONE_HOT_BLOCKS * 512
    n = hdfs.total_checksums(pk)
    want = orc.batch(host, pk, n)
    plan = hdfs.Plan(gpu_ctx, pk)
    names = {97: "s4_nt_pow2only_img32_prodgrid", 98: "s4_nt_pow2only_img32_stamps_prodgrid",
             99: "s4_nt_pow2only_stamps_prodgrid"}
    stamps = torch.zeros(4 * 12 * 1024, dtype=torch.int64, device="cuda")
    for v, name in names.items():
        assert hdfs.variant_info(v) == (name, True)
        out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        plan.exec_variant(dev.data_ptr(), out.data_ptr(), v, stamps.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want), v
    plan.close()


@pytest.mark.parametrize("skew", [0, 5], ids=["aligned", "unaligned"])
def test_resident_queue_block(hdfs, gpu_ctx, orc, payload, skew):
    """One 4 MiB block (the whole one-hot region) through the resident
    queue: its kernel stages the split image too."""
    torch = _torch()
    host, dev = payload
    pk = oracle.uniform_packets(64)
    n = hdfs.total_checksums(pk)
    want = orc.batch(host[skew:], pk, n)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plan = gpu_ctx.plan(pk)
    q = plan.blocks(resident=True, idle_us=500)
    q.wait(q.submit(dev.data_ptr() + skew, out.data_ptr()))
    got = out.cpu().numpy().view(np.uint32)
    q.close()
    plan.close()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
