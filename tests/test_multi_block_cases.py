"""CPU checks of multi_block_cases.py, the case table of test_gpu_multi_block.py:
every block shape is tiles only (a shape with any other work item takes
crc32c_plan_exec_blocks' one-launch-per-block path and would test nothing of
the multi-block form), the table names every production kernel, and on 256 CUs
the selector picks each row's kernels from the row's own counts."""
from __future__ import annotations

import cold_lds_cases
import multi_block_cases as mb

NUM_CU = 256


def _block(hdfs, name, num_cu=NUM_CU):
    s = mb.SHAPES[name]
    pk = mb.packets(s.shape, s.packets_at(num_cu))
    tiles, gen = hdfs.debug_plan(pk)
    return s, pk, tiles, gen


def test_every_block_shape_is_tiles_only(hdfs):
    """At least one tile and no gen item (no packet in cold_lds_cases.packets' layout gives seg items or
    constant runs), and the trait bits the table states."""
    for name in mb.SHAPES:
        for num_cu in (NUM_CU, 304, 64):
            s, pk, tiles, gen = _block(hdfs, name, num_cu)
            assert tiles.size >= 1 and gen.size == 0, (name, num_cu, tiles.size, gen.size)
            assert hdfs.debug_packets_flags(pk) == (s.general, s.needs_z), (name, num_cu)
    assert {c.shape for c in mb.CASES} == set(mb.SHAPES)


def test_table_names_every_production_kernel():
    assert set(mb.KERNELS) == {k for c in mb.CASES for k, _, _ in c.launches}
    want = set()
    for t, w, m in cold_lds_cases.KERNELS.values():
        want |= {(t, w, m), (t, w, m | cold_lds_cases.VERIFY)}
    assert mb.kernels_named() == want and len(want) == 22
    assert len({c.id for c in mb.CASES}) == len(mb.CASES)


def test_alignment_patterns():
    """ONE_OFF: exactly one block, neither the first nor the lowest-addressed of its launch; block 0 is
    never the lowest-addressed of a launch of several blocks; slots are a permutation."""
    for m in (3, 4, 5, 8, 15, 22, 30, 31, 32, 33, 65):
        slots = [mb.slot_of(b, m) for b in range(m)]
        assert sorted(slots) == list(range(m))
        for first, count in mb.launches_of(m):
            if count > 1:
                assert min(range(first, first + count), key=slots.__getitem__) != first, (m, first)
        if m >= 3:
            for nblocks in range(3, min(m, 32) + 1):
                (b,) = mb.misaligned_blocks(mb.ONE_OFF, nblocks, m)
                assert 0 < b < nblocks and slots[b] != min(slots[:nblocks]), (m, nblocks, b)
    assert mb.misaligned_blocks(mb.THIRD_OFF, 7, 8) == {2, 5} and not mb.misaligned_blocks(mb.ALIGNED, 7, 8)


def test_selector_picks_each_rows_kernels(hdfs):
    """Each launch of each row, from the row's own counts: blocks x tiles of a block, and the shape's
    trait bits with the shifted loads added where the launch holds a block off 16-byte alignment."""
    bands = set()
    for c in mb.CASES:
        s, pk, tiles, _ = _block(hdfs, c.shape)
        nblocks = c.nblocks_at(NUM_CU, tiles.size)
        m = mb.max_blocks(c.shape, NUM_CU, tiles.size)
        assert nblocks <= m and m % 7
        off = mb.misaligned_blocks(c.align, nblocks, m)
        launches = mb.launches_of(nblocks)
        assert len(launches) == len(c.launches), c.id
        for (first, count), (kernel, skip_z, general) in zip(launches, c.launches):
            has_off = any(first <= b < first + count for b in off)
            assert general == s.general | (mb.SHIFT if has_off else 0), (c.id, first)
            assert skip_z == int(not s.needs_z), c.id
            t, w, mode = mb.KERNELS[kernel]
            for verify in (False, True):
                b = hdfs.debug_select_build(count * tiles.size, 0, 0, 0, general, verify, NUM_CU)
                assert b.kernel == (t, w, mode | (mb.VERIFY if verify else 0)), (c.id, first, b.kernel)
        if c.count[0] != "n":
            bands.add(c.count)
    # the band walk: the last count in and the first count past every threshold
    assert bands == {(how, m) for how in ("in", "past") for m in (2, 3, 6, 16)}
    assert {c.flags for c in mb.CASES} == {0, mb.CRC32 | mb.BE}
