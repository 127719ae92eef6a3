"""The case table of test_gpu_multi_block.py: which multi-block call
(crc32c_plan_exec_blocks / crc32c_plan_verify_blocks: one block's plan over up
to 32 blocks per launch) reaches which production kernel, in which tile form.

Kept apart from the GPU test so that a CPU test (test_multi_block_cases.py)
can check that every block shape is tiles only, that the table names every
production kernel, and that the selector picks each row's kernels from the
row's own counts.  A row's block count is derived from the CU count and the
tiles of one block: it sits at the last count that stays in a build or at the
first that leaves it, and the GPU test first asserts, through
crc32c_debug_plan_blocks_launch_info, that every launch of the call selects
the kernel, the skip_z and the `general` bits the row names -- when a
threshold moves, that assertion names the row to resize.

A block is `Shape` packets as cold_lds_cases.packets lays them out; its size
follows the CU count too (about 16 C / 32 + 8 tiles of 8 KiB for the
power-of-two shapes: 136 tiles, 1.06 MiB, at 256 CUs), so that one shape walks
every band of the selector by block count alone.  136 tiles are 544 quarter
units or 272 half units a block: at 256 workgroups no count of blocks below 32
puts every block seam on the boundary between two workgroups' ranges."""
from __future__ import annotations

from typing import NamedTuple

from cold_lds_cases import KERNELS, VERIFY, Shape, packets  # noqa: F401  (re-exported for the tests)

BE = 0x1     # CRC32C_BIG_ENDIAN
CRC32 = 0x2  # CRC32C_TYPE_CRC32
MAX_LAUNCH_BLOCKS = 32
SHIFT = 2    # KParams::general: shifted loads (some block, or tile, off 16-byte alignment)


class BlockShape(NamedTuple):
    shape: Shape
    per_cu256: int  # packets of a block = per_cu256 * CUs / 256 + plus
    plus: int
    general: int    # the trait bits of the block's plan on an aligned payload
    needs_z: bool

    def packets_at(self, num_cu: int) -> int:
        return self.per_cu256 * num_cu // 256 + self.plus


# The large shapes follow the CU count (they walk the selector's bands); the
# half and padded shapes take builds of their own at any size and stay small.
SHAPES = {
    "b512": BlockShape(Shape(512), 16, 1, 0, False),
    "b1024": BlockShape(Shape(1024), 16, 1, 0, True),    # whole chunks per quarter unit
    "b4096": BlockShape(Shape(4096), 16, 1, 0, True),    # a quarter-unit build runs the tile whole; 2 chunks of a half unit each
    "b8192": BlockShape(Shape(8192), 16, 1, 0, True),    # one chunk per tile
    # every packet at offset 5 (mod 16); 3 packets whose last tile has 13 blocks
    "b512_off5": BlockShape(Shape(512, first=5, short_tail=3 * 512), 16, 1, 2, False),
    "b1536_short": BlockShape(Shape(1536, pkt_len=6144, stride=6144), 128, 1, 1, True),  # one general tile per packet
    "b1536": BlockShape(Shape(1536), 16, 1, 1, True),    # general tiles, 3 per packet, the last with a 1024-byte tail chunk
    # half tiles of whole chunks (a first chunk within 16 bytes of the payload start would be a gen item)
    "b256": BlockShape(Shape(256, first=64), 0, 3, 5, False),
    "b700": BlockShape(Shape(700, pkt_len=65100, first=64), 0, 3, 5, True),
    "b1100": BlockShape(Shape(1100, pkt_len=64900, first=64), 0, 3, 5, True),
    # padded power-of-two tiles
    "b300": BlockShape(Shape(300, pkt_len=65400, first=64), 0, 3, 11, False),
    "b1000": BlockShape(Shape(1000, first=64), 0, 3, 11, True),   # ... and a general tail tile
    "b4000": BlockShape(Shape(4000, pkt_len=64000, stride=65536, first=64), 0, 3, 11, True),
}

# Alignment patterns: which blocks sit 5 bytes past a 16-byte boundary.
ALIGNED, ONE_OFF, THIRD_OFF = "aligned", "one_off", "third_off"


def slot_of(block: int, max_blocks: int) -> int:
    """The slot of the device buffer that holds `block` when a shape's block set has max_blocks slots
    (max_blocks is no multiple of 7): block 0 is in the highest slot, and the addresses go up and down
    from there, so the lowest address of a launch (KParams::payload) is not its first block's."""
    assert max_blocks % 7 and 0 <= block < max_blocks
    return max_blocks - 1 - (7 * block) % max_blocks


def launches_of(nblocks: int):
    """[(first block, blocks)] of a call whose blocks are all within reach of each other."""
    return [(i, min(MAX_LAUNCH_BLOCKS, nblocks - i)) for i in range(0, nblocks, MAX_LAUNCH_BLOCKS)]


def misaligned_blocks(align: str, nblocks: int, max_blocks: int) -> set:
    """The blocks of a call that are 5 bytes off.  ONE_OFF: one block of the whole call, the first one
    after block 0 that is not the lowest-addressed of its launch."""
    if align == ALIGNED:
        return set()
    if align == THIRD_OFF:
        return {b for b in range(nblocks) if b % 3 == 2}
    assert align == ONE_OFF and nblocks >= 3
    lowest = min(range(min(nblocks, MAX_LAUNCH_BLOCKS)), key=lambda b: slot_of(b, max_blocks))
    return {1 if lowest != 1 else 2}


class Case(NamedTuple):
    shape: str      # SHAPES key
    count: tuple    # ("n", k): k blocks; ("in", m): the last count of at most m * CUs tiles; ("past", m): the next one
    align: str
    launches: tuple  # per launch of the call: (KERNELS key exec and verify (its twin) must select, skip_z, general)
    flags: int = 0

    @property
    def id(self) -> str:
        return "%s-%s%d-%s%s" % (self.shape, self.count[0], self.count[1], self.align, "-crc32be" if self.flags else "")

    def nblocks_at(self, num_cu: int, block_tiles: int) -> int:
        how, m = self.count
        if how == "n":
            return m
        last_in = m * num_cu // block_tiles
        assert 1 <= last_in < MAX_LAUNCH_BLOCKS, (self.id, "the band ends outside one launch: resize the shape", last_in)
        return last_in + (how == "past")


def _c(shape, count, align, *launches, flags=0):
    return Case(shape, count, align, tuple(launches), flags)


def n(k):
    return ("n", k)


def last_in(m):
    return ("in", m)


def past(m):
    return ("past", m)


# The selector's bands (csrc/plan_select.h) end at 2, 3, 6 and 16 tiles per CU.
CASES = [
    # bpc 512, whole aligned packets: no Z, through every band by block count
    _c("b512", n(1), ALIGNED, ("one_block8", 1, 0)),
    _c("b512", last_in(2), ALIGNED, ("one_block8", 1, 0)),
    _c("b512", last_in(2), ONE_OFF, ("quarter_early", 1, 2)),
    _c("b512", past(2), ALIGNED, ("quarter", 1, 0)),
    _c("b512", last_in(3), ALIGNED, ("quarter", 1, 0)),
    _c("b512", last_in(3), ONE_OFF, ("quarter", 1, 2)),
    _c("b512", past(3), ALIGNED, ("halves", 1, 0)),
    _c("b512", last_in(6), ALIGNED, ("halves", 1, 0)),
    _c("b512", last_in(6), THIRD_OFF, ("halves", 1, 2)),
    _c("b512", past(6), ALIGNED, ("small", 1, 0)),
    _c("b512", last_in(16), ALIGNED, ("small", 1, 0)),
    _c("b512", last_in(16), ONE_OFF, ("small", 1, 2)),
    _c("b512", past(16), ALIGNED, ("bulk", 1, 0)),
    _c("b512", n(32), ALIGNED, ("bulk", 1, 0)),
    _c("b512", n(32), ONE_OFF, ("shift", 1, 2)),
    _c("b512", n(33), ALIGNED, ("bulk", 1, 0), ("one_block8", 1, 0)),
    _c("b512", n(65), THIRD_OFF, ("shift", 1, 2), ("shift", 1, 2), ("one_block8", 1, 0)),  # (block 64 is aligned)
    # lg > 0: the Z section
    _c("b1024", last_in(2), ALIGNED, ("one_block8", 0, 0)),
    _c("b1024", last_in(3), ALIGNED, ("quarter", 0, 0)),
    _c("b1024", last_in(6), ONE_OFF, ("halves", 0, 2)),
    _c("b1024", n(32), ALIGNED, ("bulk", 0, 0)),
    _c("b4096", last_in(3), ONE_OFF, ("quarter", 0, 2)),
    _c("b4096", last_in(6), ALIGNED, ("halves", 0, 0)),
    _c("b4096", n(32), ALIGNED, ("bulk", 0, 0)),
    _c("b8192", last_in(16), ALIGNED, ("small", 0, 0)),
    _c("b8192", n(32), ALIGNED, ("bulk", 0, 0), flags=CRC32 | BE),
    _c("b8192", n(33), THIRD_OFF, ("shift", 0, 2), ("quarter_early", 0, 2), flags=CRC32 | BE),  # (block 32 is off)
    # every tile of the shape off 16-byte alignment, a 13-block last tile
    _c("b512_off5", n(3), ALIGNED, ("quarter_early", 1, 2)),
    _c("b512_off5", n(32), THIRD_OFF, ("shift", 1, 2)),
    # general tiles
    _c("b1536", n(3), ALIGNED, ("quarter_early", 0, 1)),
    _c("b1536", last_in(3), ONE_OFF, ("quarter", 0, 3)),
    _c("b1536", last_in(6), ALIGNED, ("halves", 0, 1)),
    _c("b1536", n(32), THIRD_OFF, ("small", 0, 3)),
    _c("b1536_short", n(32), ALIGNED, ("gitems", 0, 1)),
    _c("b1536_short", n(32), ONE_OFF, ("both_hoist", 0, 3)),
    # half tiles: builds of their own at any size
    _c("b256", n(3), ALIGNED, ("half", 1, 5)),
    _c("b256", n(32), ONE_OFF, ("half_shift", 1, 7)),
    _c("b700", n(3), ONE_OFF, ("half_shift", 0, 7)),
    _c("b700", n(32), ALIGNED, ("half", 0, 5)),
    _c("b1100", n(3), ALIGNED, ("half", 0, 5)),
    _c("b1100", n(32), THIRD_OFF, ("half_shift", 0, 7)),
    # padded power-of-two tiles: the hoisted both-paths build at any size
    _c("b300", n(3), THIRD_OFF, ("both_hoist", 1, 11)),
    _c("b300", n(32), ALIGNED, ("both_hoist", 1, 11)),
    _c("b1000", n(3), ALIGNED, ("both_hoist", 0, 11)),
    _c("b1000", n(32), ONE_OFF, ("both_hoist", 0, 11)),
    _c("b4000", n(3), ONE_OFF, ("both_hoist", 0, 11)),
    _c("b4000", n(32), THIRD_OFF, ("both_hoist", 0, 11)),
]


def max_blocks(shape: str, num_cu: int, block_tiles: int) -> int:
    """The slots a shape's block set needs: the most blocks any of its rows takes, made no multiple of 7."""
    m = max(c.nblocks_at(num_cu, block_tiles) for c in CASES if c.shape == shape)
    return m + (m % 7 == 0)


def kernels_named():
    """(threads, waves per SIMD, mode) of every kernel the table names, exec and verify."""
    out = set()
    for c in CASES:
        for k, _, _ in c.launches:
            t, w, m = KERNELS[k]
            out |= {(t, w, m), (t, w, m | VERIFY)}
    return out
