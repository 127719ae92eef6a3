"""CPU checks of stray_store.py, the helpers and case table of
test_gpu_stray_store.py: the sweep's families hold every tile the table
claims, a gapped batch plans like the gap-free one, the bands select the
builds they name at 256 CUs, and the checker fails on one changed word."""
from __future__ import annotations

import numpy as np
import pytest

import cold_lds_cases
import stray_store as ss


def _facts(hdfs, pk):
    tiles, gen = hdfs.debug_plan(pk)
    return ss.tile_facts(tiles), gen


@pytest.mark.parametrize("off5", [False, True], ids=["aligned", "off5"])
def test_families_hold_every_tile_count(hdfs, off5):
    """Through debug_plan and the meta layout of csrc/plan.h: every (form, lg or
    M, count) of the table occurs, each bpc of the half and general families
    with its own pad; the 3-byte tails are GenItems, the 4-byte and bpc - 1
    tails of the general family ride in general tiles."""
    have = {}
    for name in ss.FAMILIES:
        facts, gen = _facts(hdfs, ss.family_packets(name, off5))
        have[name] = (set(facts), gen)
    pow2 = {(lg, c) for f, lg, c, _ in have["pow2"][0] if f == "pow2"}
    assert pow2 == {(lg, c) for lg in range(5) for c in range(1, (16 >> lg) + 1)}
    assert all(f == "pow2" for f, _, _, _ in have["pow2"][0]), "the pow2 part must hold no general tile"
    # every nb in 1..16 at bpc 512, and a tile of 1 chunk behind a full one at every lg
    assert {c for lg, c in pow2 if lg == 0} == set(range(1, 17))
    # the bpc - 1 tails behind bpc 1024..8192: general tiles of k = 2^lg blocks per chunk, every count
    tails = {(k, c, tl) for f, k, c, tl in have["pow2_tail"][0] if f == "general"}
    assert tails == {(1 << lg, c, (512 << lg) - 1) for lg in range(1, 5) for c in range(1, (16 >> lg) + 1)}
    padded = {(lg, c) for f, lg, c, _ in have["padded"][0] if f == "padded"}
    assert padded == {(lg, c) for lg in range(5) for c in range(1, (16 >> lg) + 1)}
    half = {(m, c) for f, m, c, _ in have["half"][0] if f == "half"}
    assert half == {(m, c) for m, top in ((0, 32), (1, 10), (2, 6)) for c in range(1, top + 1)}
    tiles, _ = hdfs.debug_plan(ss.family_packets("half", off5))
    for bpc in ss.FAMILIES["half"].counts:  # (both bpc of every M: their own padh)
        padh = 256 - (bpc - 512 * (bpc // 512))
        got = {int(t["meta"]) & 255 for t in tiles if (int(t["meta"]) >> 30) == 1 and
               (int(t["meta"]) >> 18) & 511 == padh and (int(t["meta"]) >> 8) & 255 == bpc // 512}
        assert got == set(range(1, {0: 32, 1: 10, 2: 6}[bpc // 512] + 1)), bpc
    general = {(k, c) for f, k, c, _ in have["general"][0] if f == "general"}
    assert general >= {(-(-bpc // 512), c) for bpc in ss.FAMILIES["general"].counts for c in range(1, 17)}
    gtails = {(k, tl) for f, k, _, tl in have["general"][0] if f == "general" and tl}
    assert gtails == {(-(-bpc // 512), tl) for bpc in ss.FAMILIES["general"].counts for tl in (4, bpc - 1)}
    for name in ("pow2", "padded", "half", "general"):
        gen = have[name][1]
        assert (gen["len"] == 3).sum() == sum(len(c) for c in ss.FAMILIES[name].counts.values()), name
    # one ballast packet is one tile of the family's first bpc, and nothing else
    for name, (bpc, chunks) in ss.BALLAST.items():
        pk = ss.family_packets(name, off5)
        both = ss.with_ballast(name, pk, 3)
        assert bpc == next(iter(ss.FAMILIES[name].counts)) and both.size == pk.size + 3
        t0, g0 = hdfs.debug_plan(pk)
        t1, g1 = hdfs.debug_plan(both)
        assert t1.size == t0.size + 3 and g1.size == g0.size, name
        assert len({(int(t["src"]), int(t["meta"])) for t in t1[-3:]}) == 1 and int(t1[-1]["src"]) % 16 == 0
        form = ss.tile_facts(t1[-1:])[0]
        assert form[0] == ss.FAMILIES[name].form and form[2] == chunks and form[3] == 0, (name, form)


def test_packets_sit_where_the_table_says():
    for name in ss.FAMILIES:
        for off5 in (False, True):
            pk = ss.family_packets(name, off5)
            assert (pk["payload_off"] % 16 == (5 if off5 else 0)).all() and int(pk["payload_off"].min()) >= ss.FIRST
            ends = pk["payload_off"] + pk["len"]
            assert (pk["payload_off"][1:] >= ends[:-1]).all(), "packets overlap in the payload"
            assert (pk["out_idx"] == ss.dense(pk)["out_idx"]).all()
    assert ss.ptr_off(True) == 5 and ss.ptr_off(False) == 0


@pytest.mark.parametrize("name", sorted(ss.FAMILIES))
def test_gapped_batch_plans_like_the_gap_free_one(hdfs, name):
    """Same tiles and gen items, except for `out`; and `out` moves by exactly the
    gaps before the item's packet."""
    pk = ss.with_ballast(name, ss.family_packets(name, True), 5)
    gp = ss.gapped(pk)
    per = ss.nchunks(pk)
    assert (gp["out_idx"] == pk["out_idx"] + np.uint64(ss.GAP) * (np.arange(pk.size, dtype=np.uint64) + 1)).all()
    assert hdfs.total_checksums(gp) == hdfs.total_checksums(pk) + ss.GAP * pk.size
    assert int(per.sum()) == hdfs.total_checksums(pk)
    (t0, g0), (t1, g1) = hdfs.debug_plan(pk), hdfs.debug_plan(gp)
    assert t0.size == t1.size and g0.size == g1.size
    for a, b in ((t0, t1), (g0, g1)):
        for field in a.dtype.names:
            if field != "out":
                assert (a[field] == b[field]).all(), (name, field)
        # the packet of a dense index, hence the gaps before it
        which = np.searchsorted(pk["out_idx"], a["out"].astype(np.uint64), side="right")
        assert (b["out"].astype(np.uint64) == a["out"].astype(np.uint64) + np.uint64(ss.GAP) * which).all(), name
    # the plan's flags do not depend on the layout of the checksums
    assert hdfs.debug_packets_flags(pk) == hdfs.debug_packets_flags(gp)
    cov = ss.covered_mask(hdfs.total_checksums(gp), gp)
    assert int(cov.sum()) == int(per.sum()) and not cov[:ss.GAP].any()
    idx = np.flatnonzero(cov)
    runs = np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1)
    assert len(runs) == pk.size and all(r[0] - q[-1] - 1 == ss.GAP for q, r in zip(runs, runs[1:]))


def test_sweep_bands_name_every_build_and_select_it_at_256_cus(hdfs):
    """The table's bands name all eleven exec builds of cold_lds_cases.KERNELS,
    all four phases occur in every family, and at 256 CUs select_plan_build
    chooses the named build (exec and its verify twin) for every case.  (The
    GPU test asserts the same through launch_info at the device's CU count.)"""
    assert {c.band.kernel for c in ss.SWEEP} == set(cold_lds_cases.KERNELS)
    assert len({c.id for c in ss.SWEEP}) == len(ss.SWEEP)
    for name in ss.FAMILIES:
        assert {c.phase for c in ss.SWEEP if c.family == name} == {0, 1, 2, 3}, name
    num_cu = 256
    for c in ss.SWEEP:
        pk = ss.family_packets(c.family, c.off5)
        tiles, gen = hdfs.debug_plan(pk)
        nb = c.band.ballast(num_cu, tiles.size, gen.size)
        general, _ = hdfs.debug_packets_flags(ss.gapped(ss.with_ballast(c.family, pk, nb)))
        if c.off5:
            general |= 2  # (kGeneralShift: the device pointer is off 16-byte alignment)
        t, w, m = cold_lds_cases.KERNELS[c.band.kernel]
        for verify in (False, True):
            b = hdfs.debug_select_build(tiles.size + nb, gen.size, 0, 0, general, verify, num_cu)
            assert b.kernel == (t, w, m | (cold_lds_cases.VERIFY if verify else 0)), (c.id, verify, b.kernel)


def test_assert_image_names_guard_gap_and_covered_words():
    pk = ss.gapped(ss.dense(np.array([(0, 0, 1024, 512), (1024, 0, 700, 512)], dtype=ss.oracle.PACKET_DTYPE)))
    n = int((pk["out_idx"] + ss.nchunks(pk)).max())
    assert n == 64 + 2 + 64 + 2
    want = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(1)
    for fill in ss.FILLS:
        for phase in range(4):
            img = ss.expected_image(n, fill, pk, want, phase)
            lead, total = ss.layout(n, phase)
            assert img.words.size == total and lead == ss.GUARD_WORDS + phase and total - lead - n >= ss.GUARD_WORDS
            assert (lead * 4) % 16 == 4 * phase
            assert int(img.covered.sum()) == 4 and (img.words[lead:lead + n][img.covered] == want[img.covered]).all()
            assert (np.delete(img.words, lead + np.flatnonzero(img.covered)) == fill).all()
            ss.assert_image(img.words.copy(), img, "untouched")
            spots = {0: "leading guard", lead - 1: "leading guard, 1 words before", lead: "gap, index 0",
                     lead + 64: "covered index 64", lead + 65: "covered index 65", lead + 66: "gap, index 66",
                     lead + n - 1: "covered index %d" % (n - 1), lead + n: "trailing guard, 1 words past",
                     total - 1: "trailing guard"}
            for at, where in spots.items():
                got = img.words.copy()
                got[at] ^= np.uint32(0x00010000)
                with pytest.raises(AssertionError) as e:
                    ss.assert_image(got, img, "one word changed")
                msg = str(e.value)
                assert "1 words differ" in msg and "word %d (%s" % (at, where) in msg, msg
    # a store of the fill's own value into a gap shows under the other fill
    a, b = (ss.expected_image(n, f, pk, want) for f in ss.FILLS)
    stray = a.words.copy()
    stray[a.lead + 3] = ss.FILLS[1]
    with pytest.raises(AssertionError):
        ss.assert_image(stray, a, "a stray zero")
    with pytest.raises(AssertionError):
        ss.assert_image(a.words, b, "the other fill's image")
    with pytest.raises(AssertionError):  # overlapping packets are a mistake of the test, not a layout
        ss.covered_mask(8, np.array([(0, 0, 1024, 512), (0, 1, 1024, 512)], dtype=ss.oracle.PACKET_DTYPE))
