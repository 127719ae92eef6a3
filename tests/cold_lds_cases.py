"""The case table of test_gpu_cold_lds.py: which batch reaches which of the
production kernels, and whether its launch stages the Z^(512 s) section.

Kept apart from the GPU tests so that a CPU test (test_host_lib.py) can check
that the table names every production kernel.  Packet counts are derived from
the CU count: a case sits at the last batch size that stays in a build or at
the first that leaves it, and the GPU test first asserts, through
crc32c_debug_plan_launch_info, that the launch path chooses the kernel and the
skip_z the case names -- when a threshold moves, that assertion names the case
to resize."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import oracle

# hdfs_crc32c_plan_kernel<threads, waves per SIMD, mode> of each production
# build's exec form (csrc/plan_select.h mode bits; the verify twin is mode | 64).
NP = 2097152  # no padded power-of-two tiles
VERIFY = 64
KERNELS = {
    "bulk": (768, 3, 3),                      # full image, power-of-two tiles only
    "both_hoist": (768, 3, 131331),           # full image, general tiles + shifted loads, hoisted
    "gitems": (768, 3, 33027),                # full image, general tiles, no shifted loads
    "shift": (768, 3, 65795),                 # full image, shifted loads, no general tiles
    "small": (768, 3, 771 + NP),              # compact image, whole tiles
    "halves": (768, 3, 21251 + NP),           # compact image, half units
    "quarter": (768, 3, 4867 + NP),           # compact image, quarter units
    "quarter_early": (768, 3, 5891 + NP),     # ... first unit's loads before the staging
    "one_block8": (512, 2, 5635),             # ... without the general-tile code, 8 waves
    "half": (768, 3, 1081603),                # half tiles, no shifted loads
    "half_shift": (768, 3, 1179907),          # half tiles with shifted loads
}

PKT = 65536


class Shape(NamedTuple):
    bpc: int
    pkt_len: int = PKT      # bytes per packet
    stride: int = PKT       # payload distance between packets
    first: int = 0          # payload offset of packet 0
    ptr_off: int = 0        # bytes added to the device payload pointer itself
    short_tail: int = 0     # the last 3 packets are this many bytes shorter (partial last tiles)


SHAPES = {
    "b512": Shape(512),
    "b1024": Shape(1024),
    "b4096": Shape(4096),
    # every packet at offset 5 (mod 16); 3 packets whose last tile has 13 blocks
    "b512_off5": Shape(512, first=5, short_tail=3 * 512),
    "b1536": Shape(1536),                                   # general tiles (3 per packet) with a 1024-byte tail
    "b1536_ptr5": Shape(1536, ptr_off=5),
    "b1536_short": Shape(1536, pkt_len=6144, stride=6144),  # one general tile of 4 chunks per packet
    "b1536_short_ptr5": Shape(1536, pkt_len=6144, stride=6144, ptr_off=5),
    # half tiles of whole chunks (a first chunk within 16 bytes of the payload start would be a gen item)
    "b256": Shape(256, first=64),                           # M = 0
    "b256_off5": Shape(256, first=69),
    "b256_ptr5": Shape(256, first=64, ptr_off=5),
    "b700": Shape(700, pkt_len=65100, first=64),            # M = 1
    "b300": Shape(300, pkt_len=65400, first=64),            # padded lg-0 tiles alone
    "b1000": Shape(1000, first=64),                         # padded lg-1 tiles and a general tail tile
}


class Case(NamedTuple):
    shape: str
    per_cu8: int    # packets = per_cu8 * CUs / 8 + plus (per_cu8 tiles per CU at 8 tiles per packet)
    plus: int
    kernel: str     # KERNELS key both exec and verify (its twin) must select
    skip_z: int
    general: int    # KParams::general bits

    @property
    def id(self) -> str:
        return "%s-%dcu8+%d" % (self.shape, self.per_cu8, self.plus)

    def packets_at(self, num_cu: int) -> int:
        return self.per_cu8 * num_cu // 8 + self.plus


def _c(shape, per_cu8, plus, kernel, skip_z, general):
    return Case(shape, per_cu8, plus, kernel, skip_z, general)


# At 256 CUs per_cu8 = 2, 3, 6, 16 are 64, 96, 192, 512 packets of 64 KiB.
CASES = [
    # bpc 512, aligned whole packets: no Z, no general-tile code, through every batch-size band
    _c("b512", 0, 1, "one_block8", 1, 0),
    _c("b512", 2, 0, "one_block8", 1, 0),
    _c("b512", 2, 1, "quarter", 1, 0),
    _c("b512", 3, 0, "quarter", 1, 0),
    _c("b512", 3, 1, "halves", 1, 0),
    _c("b512", 6, 0, "halves", 1, 0),
    _c("b512", 6, 1, "small", 1, 0),
    _c("b512", 16, 0, "small", 1, 0),
    _c("b512", 16, 1, "bulk", 1, 0),
    # lg > 0: the Z section is needed (bpc 1024: whole chunks per quarter unit; 4096: unit 0 runs the tile)
    _c("b1024", 2, 0, "one_block8", 0, 0),
    _c("b1024", 3, 0, "quarter", 0, 0),
    _c("b1024", 6, 0, "halves", 0, 0),
    _c("b4096", 2, 0, "one_block8", 0, 0),
    _c("b4096", 3, 0, "quarter", 0, 0),
    _c("b4096", 6, 0, "halves", 0, 0),
    # bpc 512 off 16-byte alignment: shifted loads, still no Z
    _c("b512_off5", 2, 0, "quarter_early", 1, 2),
    _c("b512_off5", 3, 0, "quarter", 1, 2),
    _c("b512_off5", 6, 0, "halves", 1, 2),
    _c("b512_off5", 16, 0, "small", 1, 2),
    _c("b512_off5", 16, 1, "shift", 1, 2),
    # bpc 1536: general tiles, 3 per 64 KiB packet -- 513 packets are 1539 tiles, still a small batch;
    # the full-image general builds start above 16 items per CU: packets of one tile each
    _c("b1536", 2, 0, "quarter_early", 0, 1),
    _c("b1536", 16, 1, "small", 0, 1),
    _c("b1536_ptr5", 16, 1, "small", 0, 3),
    _c("b1536_short", 128, 8, "gitems", 0, 1),
    _c("b1536_short_ptr5", 128, 8, "both_hoist", 0, 3),
    # half tiles: builds of their own at any size
    _c("b256", 0, 8, "half", 1, 5),
    _c("b256", 16, 1, "half", 1, 5),
    _c("b256_off5", 0, 8, "half", 1, 5),
    _c("b256_off5", 16, 1, "half", 1, 5),
    _c("b256_ptr5", 0, 8, "half_shift", 1, 7),
    _c("b256_ptr5", 16, 1, "half_shift", 1, 7),
    _c("b700", 0, 8, "half", 0, 5),
    _c("b700", 16, 1, "half", 0, 5),
    # padded power-of-two tiles: the hoisted both-paths build at any size
    _c("b300", 0, 8, "both_hoist", 1, 11),
    _c("b300", 16, 1, "both_hoist", 1, 11),
    _c("b1000", 0, 8, "both_hoist", 0, 11),
]

# Kernels (exec forms) the write-plan and alternating-polynomial tests of
# test_gpu_cold_lds.py run, beside CASES: a zero-fill buffer then aligned data
# (tiles + constant runs), constant runs alone, and the 64-packet bpc-1024 batch.
OTHER_KERNELS = ("one_block8",)


def packets(shape: Shape, n: int) -> np.ndarray:
    pk = oracle.uniform_packets(n, pkt_len=shape.pkt_len, bpc=shape.bpc, stride=shape.stride)
    pk["payload_off"] += shape.first
    if shape.short_tail:
        pk["len"][-3:] -= shape.short_tail
    per = (pk["len"].astype(np.uint64) + np.uint64(shape.bpc - 1)) // np.uint64(shape.bpc)
    pk["out_idx"] = np.concatenate([[0], np.cumsum(per)[:-1]]).astype(np.uint64)  # no gap in the checksum array
    return pk


def kernels_named():
    """(threads, waves per SIMD, mode) of every kernel the tables name, exec and verify."""
    names = {c.kernel for c in CASES} | set(OTHER_KERNELS)
    out = set()
    for k in names:
        t, w, m = KERNELS[k]
        out |= {(t, w, m), (t, w, m | VERIFY)}
    return out
