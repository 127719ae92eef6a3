"""Helpers and the case table of test_gpu_stray_store.py: outputs between
guard words and with gaps inside, so that a store by a lane that should have
been masked off, or past either end of the checksum array, lands on a word
nothing else writes and is seen on every run.

Plain Python, no GPU at import (torch is imported where device memory is
allocated).  A CPU test (test_stray_store_cases.py) checks that the table
below holds the tiles it claims, that a gapped batch plans like the gap-free
one, and that the checker fails when one word is changed.

The partial-tile sweep has one family per tile form (csrc/plan.h).  Each holds
the smallest packets that contain every count of chunks a tile of that form
can hold, and one more, each with the tails of TAILS.  The power-of-two family
of the table comes in two parts, because a tail longer than one 512-byte block
behind power-of-two chunks rides in a general tile and a batch with general
tiles never runs the builds without their code: `pow2` (no tail, 3 bytes, 4
bytes and, at bpc 512, bpc - 1) reaches one_block8 and bulk, `pow2_tail` (the
bpc - 1 tails of bpc 1024..8192) reaches gitems."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import oracle

GUARD_WORDS = 64           # guard words on each side of a GuardedWords (a multiple of 4)
FILLS = (0xEEEEEEEE, 0x00000000)  # a stray store of any value differs from one of them
GAP = 64                   # a wave has 64 lanes: a stray t.out + lane store lands in a gap or a guard
FIRST = 64                 # payload offset of a family's first packet (half tiles: >= 64 bytes in)
SLACK = 8192               # payload bytes behind the last packet


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def layout(n: int, phase: int):
    """(words before the first output word, words in all) of a GuardedWords."""
    assert 0 <= phase <= 3
    lead = GUARD_WORDS + phase
    return lead, lead + n + GUARD_WORDS + (4 - phase)


class GuardedWords:
    """n uint32 words of device memory, the first one `phase` words (0..3) past
    a 16-byte boundary, between two runs of at least GUARD_WORDS guard words;
    one int32 allocation filled with `fill`."""

    def __init__(self, n: int, fill: int, phase: int = 0):
        torch = _torch()
        self.n, self.fill, self.phase = n, fill & 0xFFFFFFFF, phase
        self.lead, self.total = layout(n, phase)
        self.t = torch.full((self.total,), _i32(fill), dtype=torch.int32, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * self.lead
        assert self.ptr % 16 == 4 * phase

    def refill(self, fill: int | None = None):
        if fill is not None:
            self.fill = fill & 0xFFFFFFFF
        self.t.fill_(_i32(self.fill))

    def upload(self, whole: np.ndarray):
        """The whole allocation, guards included, from a host array (an expected_image's words)."""
        torch = _torch()
        whole = np.ascontiguousarray(whole, dtype=np.uint32)
        assert whole.size == self.total
        self.t.copy_(torch.from_numpy(whole.view(np.int32).copy()))

    def read(self) -> np.ndarray:
        """The whole allocation, guards included (a host copy; a device-to-host copy, no kernel)."""
        return self.t.cpu().numpy().view(np.uint32).copy()


class Image(NamedTuple):
    words: np.ndarray    # the whole array as it must read back, guards included
    lead: int            # guard words before index 0
    n: int               # words between the guards
    covered: np.ndarray  # bool[n]: the indices the packets cover


def covered_mask(n: int, pk) -> np.ndarray:
    """bool[n]: True at every checksum index of the packets (None: every index)."""
    if pk is None:
        return np.ones(n, bool)
    m = np.zeros(n, bool)
    for p in pk:
        if int(p["len"]):
            a = int(p["out_idx"])
            b = a + -(-int(p["len"]) // int(p["bpc"]))
            assert b <= n and not m[a:b].any(), "packets overlap or pass the end of the array"
            m[a:b] = True
    return m


def expected_image(n: int, fill: int, pk, want: np.ndarray, phase: int = 0) -> Image:
    """The array of GuardedWords(n, fill, phase) as it must read back: `fill`
    everywhere except the indices the packets cover (pk None: all n), which
    hold the oracle's values want[index]."""
    lead, total = layout(n, phase)
    words = np.full(total, fill & 0xFFFFFFFF, np.uint32)
    cov = covered_mask(n, pk)
    want = np.asarray(want, dtype=np.uint32)
    assert want.size == n
    words[lead:lead + n][cov] = want[cov]
    words.setflags(write=False)
    return Image(words, lead, n, cov)


def place(image: Image, i: int) -> str:
    """Where word i of the whole array lies: guard, gap or covered index."""
    if i < image.lead:
        return "leading guard, %d words before index 0" % (image.lead - i)
    if i >= image.lead + image.n:
        return "trailing guard, %d words past the last index" % (i - image.lead - image.n + 1)
    k = i - image.lead
    return ("covered index %d" if image.covered[k] else "gap, index %d") % k


def assert_image(got: np.ndarray, image: Image, what):
    """The whole array, guards included, against the image; a failure names the
    first offending words and where each lies."""
    got = np.asarray(got).view(np.uint32).reshape(-1)
    assert got.size == image.words.size, (what, got.size, image.words.size)
    bad = np.flatnonzero(got != image.words)
    if bad.size == 0:
        return
    lines = ["%s: %d words differ" % (what, bad.size)]
    for i in bad[:8].tolist():
        lines.append("  word %d (%s): got %08x, want %08x" % (i, place(image, i), int(got[i]), int(image.words[i])))
    raise AssertionError("\n".join(lines))


def nchunks(pk) -> np.ndarray:
    return (pk["len"].astype(np.uint64) + pk["bpc"].astype(np.uint64) - np.uint64(1)) // pk["bpc"].astype(np.uint64)


def dense(pk) -> np.ndarray:
    """out_idx from 0 without gaps, in packet order."""
    pk = pk.copy()
    per = nchunks(pk)
    pk["out_idx"] = np.concatenate([[0], np.cumsum(per)[:-1]]).astype(np.uint64)
    return pk


def gapped(pk, gap: int = GAP, lead: int = GAP) -> np.ndarray:
    """out_idx rewritten, in packet order, so that `lead` uncovered words start
    the array and `gap` uncovered words precede every later packet's range."""
    pk = pk.copy()
    per = nchunks(pk)
    start = np.concatenate([[0], np.cumsum(per + np.uint64(gap))[:-1]]).astype(np.uint64)
    pk["out_idx"] = start + np.uint64(lead)
    return pk


# ---- the partial-tile sweep ----------------------------------------------------
TAILS = ("none", 3, 4, "bpc-1")  # 3: a GenItem; 4: the smallest tail a general tile carries


class Family(NamedTuple):
    form: str            # pow2 | padded | half | general (csrc/plan.h)
    counts: dict         # bpc -> the chunk counts of its packets
    tails: tuple         # of TAILS


def _lg(k: int) -> int:
    return k.bit_length() - 1


FAMILIES = {
    # 1 .. 16 >> lg chunks, plus one tile and 1 chunk
    "pow2": Family("pow2", {512 << lg: range(1, (16 >> lg) + 2) for lg in range(5)}, ("none", 3, 4, "bpc-1:one-block")),
    "pow2_tail": Family("pow2", {512 << lg: range(1, (16 >> lg) + 2) for lg in range(1, 5)}, ("bpc-1",)),
    "padded": Family("padded", {bpc: range(1, (16 >> lg) + 2) for lg, bpc in enumerate((300, 1000, 1800, 3600, 7700))},
                     TAILS),
    "half": Family("half", {100: range(1, 34), 256: range(1, 34), 700: range(1, 12), 768: range(1, 12),
                            1100: range(1, 8), 1280: range(1, 8)}, TAILS),
    "general": Family("general", {bpc: range(1, 18) for bpc in (1536, 2560, 3000, 5000, 7000)}, TAILS),
}

# One ballast packet is one tile of the family's first bpc: (bpc, chunks).
BALLAST = {"pow2": (512, 16), "pow2_tail": (1024, 8), "padded": (300, 16), "half": (100, 32), "general": (1536, 16)}


def _tail_bytes(tail, bpc: int):
    if tail == "none":
        return 0
    if tail == "bpc-1":
        return bpc - 1
    if tail == "bpc-1:one-block":  # (behind power-of-two chunks a tail of at most 512 bytes is a GenItem)
        return bpc - 1 if bpc - 1 <= 512 else None
    return tail


def family_packets(name: str, off5: bool = False) -> np.ndarray:
    """The family's packets, checksums from index 0 without gaps, each packet on
    16-byte alignment from FIRST on (off5: 5 bytes past it; the GPU test then
    also moves the device pointer by 5, ptr_off(off5))."""
    fam = FAMILIES[name]
    rows, pos = [], FIRST
    for bpc, counts in fam.counts.items():
        for c in counts:
            for tail in fam.tails:
                tl = _tail_bytes(tail, bpc)
                if tl is None:
                    continue
                plen = c * bpc + tl
                rows.append((pos + (5 if off5 else 0), 0, plen, bpc))
                pos = (pos + plen + 5 + 15) // 16 * 16
    return dense(np.array(rows, dtype=oracle.PACKET_DTYPE))


def ptr_off(off5: bool) -> int:
    return 5 if off5 else 0


def with_ballast(name: str, pk: np.ndarray, nballast: int) -> np.ndarray:
    """pk followed by nballast whole, aligned one-tile packets of the family's
    first bpc that all read the same payload region behind the family's
    packets (dense out_idx)."""
    if nballast <= 0:
        return pk
    bpc, chunks = BALLAST[name]
    at = (int((pk["payload_off"] + pk["len"]).max()) + 15) // 16 * 16
    b = np.zeros(nballast, dtype=oracle.PACKET_DTYPE)
    b["payload_off"], b["len"], b["bpc"] = at, bpc * chunks, bpc
    return dense(np.concatenate([pk, b]))


def payload_bytes(pk: np.ndarray, off5: bool) -> int:
    return (int((pk["payload_off"] + pk["len"]).max()) + ptr_off(off5) + SLACK + 15) // 16 * 16


class Band(NamedTuple):
    name: str       # first | quarter | halves | small | large
    kernel: str     # cold_lds_cases.KERNELS key exec and verify (its twin) must select

    def ballast(self, num_cu: int, ntiles: int, ngen: int) -> int:
        """Ballast tiles that put a family of ntiles tiles and ngen gen items at the
        last batch size of the band (large: the first past the small batches);
        csrc/plan_select.h."""
        pairs = (ngen + 1) // 2
        target = {"first": ntiles, "quarter": 3 * num_cu, "halves": 6 * num_cu, "small": 16 * num_cu - pairs,
                  "large": 16 * num_cu - pairs + 1}[self.name]
        assert target >= ntiles, "the family alone is past this band at %d CUs" % num_cu
        return target - ntiles


def _bands(first, large):
    return (Band("first", first), Band("quarter", "quarter"), Band("halves", "halves"), Band("small", "small"),
            Band("large", large))


# (family, off5) -> the bands select_plan_build can put it in.  Half tiles and
# padded power-of-two tiles run one build at any size: the family alone and
# past 16 items per CU (workgroups that loop over several items).
BANDS = {
    ("pow2", False): _bands("one_block8", "bulk"),
    ("pow2", True): _bands("quarter_early", "shift"),
    ("pow2_tail", False): _bands("quarter_early", "gitems"),
    ("pow2_tail", True): _bands("quarter_early", "both_hoist"),
    ("general", False): _bands("quarter_early", "both_hoist"),
    ("general", True): _bands("quarter_early", "both_hoist"),
    ("padded", False): (Band("first", "both_hoist"), Band("large", "both_hoist")),
    ("padded", True): (Band("first", "both_hoist"), Band("large", "both_hoist")),
    ("half", False): (Band("first", "half"), Band("large", "half")),
    ("half", True): (Band("first", "half_shift"), Band("large", "half_shift")),
}


class SweepCase(NamedTuple):
    family: str
    off5: bool
    band: Band
    phase: int      # of the case's guarded arrays: the case's index in its family, mod 4

    @property
    def id(self) -> str:
        return "%s-%s-%s" % (self.family, "off5" if self.off5 else "aligned", self.band.name)


def sweep_cases():
    out = []
    for fam in FAMILIES:
        k = 0
        for off5 in (False, True):
            for band in BANDS[(fam, off5)]:
                out.append(SweepCase(fam, off5, band, k % 4))
                k += 1
    return out


SWEEP = sweep_cases()


# ---- tile descriptors (csrc/plan.h, FastTile::meta) ------------------------------
def tile_facts(tiles: np.ndarray):
    """[(form, lg or M or k, chunks, tail bytes)] of a debug_plan tile array."""
    out = []
    for t in tiles:
        meta, src = int(t["meta"]), int(t["src"])
        pad = (meta >> 18) & 511
        if meta & 0x80000000:
            out.append(("general", (meta >> 8) & 31, (meta >> 13) & 31, src >> 48))
        elif meta & 0x40000000:
            out.append(("half", (meta >> 8) & 255, meta & 255, 0))
        else:
            lg = (meta >> 8) & 255
            out.append(("padded" if pad else "pow2", lg, (meta & 255) >> lg, 0))
    return out
