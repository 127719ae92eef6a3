"""The AES/CTR launch sizing (csrc/aes_ctr.hip) through crc32c_debug_aes_strided_launch_info and
crc32c_debug_aes_list_launch_info, the functions the entry points size their launches with: windows,
wave units, windows per lane and grid at every threshold.  Expected figures are worked out here from
the geometry hook's units.  No GPU."""
from __future__ import annotations

import errno

import pytest

BASE = 1 << 40  # device addresses are opaque to the sizing


@pytest.fixture(scope="module")
def geom(hdfs):
    return hdfs.debug_aes_geometry()


def _want(geom, num_cu, windows, wpl):
    units = -(-windows // (64 * wpl))
    wg_per_cu = geom["lanes_per_cu"] * geom["lane_bytes"] // geom["workgroup_bytes"]
    assert wg_per_cu == 2
    return {"windows": windows, "wave_units": units, "windows_per_lane": wpl, "grid": min(units, 2 * num_cu)}


@pytest.mark.parametrize("num_cu", [256, 80])
def test_windows_per_lane_thresholds(hdfs, geom, num_cu):
    """lanes, lanes + 1, 2 lanes and 2 lanes + 1 windows give a lane 1, 2, 2 and lane_bytes / 16 windows:
    one aligned segment, one 3 bytes off a boundary, and the same windows cut into list segments."""
    lanes = geom["lanes_per_cu"] * num_cu
    full = geom["lane_bytes"] // 16
    assert full > 2
    for windows, wpl in ((lanes, 1), (lanes + 1, 2), (2 * lanes, 2), (2 * lanes + 1, full)):
        want = _want(geom, num_cu, windows, wpl)
        assert hdfs.debug_aes_strided_launch_info(num_cu, BASE, 16 * windows) == want
        assert hdfs.debug_aes_strided_launch_info(num_cu, BASE + 3, 16 * windows - 3) == want
        assert hdfs.debug_aes_strided_launch_info(num_cu, BASE + 3, 16 * windows - 18) == want  # (a ragged end)
        assert hdfs.debug_aes_list_launch_info(num_cu, [(BASE, BASE, 0, 16 * windows)]) == want
        # three list segments: 100 windows at phase 5, 7 at phase 0, the rest at phase 15 with a ragged end;
        # every segment's wave units are rounded up on their own
        rest = windows - 107
        segs = [(0, BASE + 5, 9, 16 * 100 - 5), (0, BASE + (1 << 30), 0, 16 * 7), (0, BASE + (2 << 30) + 15, 3, 16 * rest - 20)]
        units = sum(-(-w // (64 * wpl)) for w in (100, 7, rest))
        assert hdfs.debug_aes_list_launch_info(num_cu, segs) == {
            "windows": windows, "wave_units": units, "windows_per_lane": wpl, "grid": min(units, 2 * num_cu)}


@pytest.mark.parametrize("num_cu", [256, 80])
def test_strided_segments(hdfs, geom, num_cu):
    """A ragged strided call (dst_stride % 16 != 0, more than one segment) is sized at phase 15 whatever
    dst's own phase; one segment, or a stride that keeps the phase, at dst's phase."""
    lanes = geom["lanes_per_cu"] * num_cu
    full = geom["lane_bytes"] // 16
    # 1000 bytes: 63 windows at phases 0 .. 8, 64 at phases 9 .. 15
    for dst_phase in (0, 5, 8, 9, 15):
        own = 63 if dst_phase <= 8 else 64
        info = hdfs.debug_aes_strided_launch_info(num_cu, BASE + dst_phase, 1000, 65, 1003)
        assert info == {"windows": 65 * 64, "wave_units": 65, "windows_per_lane": 1, "grid": 65}, dst_phase
        info = hdfs.debug_aes_strided_launch_info(num_cu, BASE + dst_phase, 1000, 65, 1008)
        assert info == {"windows": 65 * own, "wave_units": 65, "windows_per_lane": 1, "grid": 65}, dst_phase
        info = hdfs.debug_aes_strided_launch_info(num_cu, BASE + dst_phase, 1000, 1, 1003)
        assert info == {"windows": own, "wave_units": 1, "windows_per_lane": 1, "grid": 1}, dst_phase
    # the thresholds count the windows of all segments; a segment's wave units are rounded up on their own
    for nsegs, wpl in ((lanes // 64, 1), (lanes // 64 + 1, 2), (2 * lanes // 64, 2), (2 * lanes // 64 + 1, full)):
        info = hdfs.debug_aes_strided_launch_info(num_cu, BASE, 1000, nsegs, 1003)
        assert info == {"windows": 64 * nsegs, "wave_units": nsegs, "windows_per_lane": wpl,
                        "grid": min(nsegs, 2 * num_cu)}, nsegs
    # 64 KiB packets, everything aligned: 4096 windows each
    nsegs = 2 * lanes // 4096 + 1
    info = hdfs.debug_aes_strided_launch_info(num_cu, BASE, 65536, nsegs, 65536)
    assert info == {"windows": 4096 * nsegs, "wave_units": nsegs * (4096 // (64 * full)), "windows_per_lane": full,
                    "grid": 2 * num_cu}
    # nothing to do
    nothing = {"windows": 0, "wave_units": 0, "windows_per_lane": 0, "grid": 0}
    assert hdfs.debug_aes_strided_launch_info(num_cu, BASE, 0, 5, 16) == nothing
    assert hdfs.debug_aes_strided_launch_info(num_cu, BASE, 100, 0, 16) == nothing


@pytest.mark.parametrize("num_cu", [256, 80])
def test_list_zero_length_entries_add_nothing(hdfs, geom, num_cu):
    lanes = geom["lanes_per_cu"] * num_cu
    live = [(0, BASE + 7 + 4096 * i, i, 1 + 37 * i) for i in range(20)] + [(0, BASE + (1 << 30), 0, 16 * lanes)]
    holed = []
    for i, s in enumerate(live):
        holed += [(0, 0, i, 0), s] if i % 3 == 0 else [s]
    holed.append((0, BASE + 11, 0, 0))  # (a zero-length entry with a destination off a boundary)
    assert len(holed) <= geom["list_max_segments"]
    a, b = hdfs.debug_aes_list_launch_info(num_cu, live), hdfs.debug_aes_list_launch_info(num_cu, holed)
    assert a == b and a["windows_per_lane"] == 2
    windows = [(ln >> 4) + (((ln & 15) + (d & 15) + 15) >> 4) for _, d, _, ln in live]
    assert a["windows"] == sum(windows) and a["wave_units"] == sum(-(-w // 128) for w in windows)
    assert a["grid"] == min(a["wave_units"], 2 * num_cu)
    empty = {"windows": 0, "wave_units": 0, "windows_per_lane": 1, "grid": 0}
    assert hdfs.debug_aes_list_launch_info(num_cu, []) == empty
    assert hdfs.debug_aes_list_launch_info(num_cu, [(0, 0, 5, 0)] * 3) == empty


def test_grid_is_wave_units_up_to_two_workgroups_per_cu(hdfs, geom):
    for num_cu in (256, 80, 1):
        for units in (1, 2 * num_cu - 1, 2 * num_cu, 2 * num_cu + 1, 64 * num_cu):
            info = hdfs.debug_aes_strided_launch_info(num_cu, BASE, 16 * 64 * units)
            wpl = info["windows_per_lane"]
            assert info["wave_units"] == -(-units // wpl) and info["grid"] == min(info["wave_units"], 2 * num_cu)


def test_argument_errors(hdfs, geom):
    cap = geom["list_max_segments"]
    seg = (0, BASE, 0, 100)
    assert hdfs.debug_aes_list_launch_info(256, [seg] * cap)["wave_units"] == cap
    for call in (lambda: hdfs.debug_aes_list_launch_info(256, [seg] * (cap + 1)),
                 lambda: hdfs.debug_aes_list_launch_info(0, [seg]),
                 lambda: hdfs.debug_aes_strided_launch_info(0, BASE, 100),
                 lambda: hdfs.debug_aes_strided_launch_info(256, BASE, 1 << 62, 1 << 40, 16)):
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == -errno.EINVAL
