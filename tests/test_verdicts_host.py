"""crc32c_bitmap_verdicts_host (include/hdfs_crc32c.h section 6d;
csrc/verdicts_host.cpp): per-cell verdicts from a mismatch bitmap, against a
numpy oracle that shares no code with it (np.unpackbits, then per cell the
sum and the first / last flatnonzero).  No GPU.  The size and pattern tables
here are also the GPU tests' (tests/test_gpu_verify_blocks.py imports them).
Every output array sits between guard records; the bits of the bitmap's last
word at or past nsums are always set and must never count."""
from __future__ import annotations

import ctypes
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NONE = 0xFFFFFFFF
CELL_SIZES = [1, 31, 32, 33, 63, 64, 65, 258, 2047, 2048, 2049, 8192, 8193]
PATTERNS = ["empty", "ones", "first", "last", "neighbours", "half", "sparse"]
GUARD = 0xEEEEEEEE


def nsums_table(cpc: int):
    """nsums for one cell size: a ragged last cell of 1 bit, one of cpc - 1
    bits, one single ragged cell (nsums < cpc), whole cells only, and 0."""
    ns = {3 * cpc + 1, 2 * cpc + max(cpc - 1, 1), max(cpc - 1, 1), 4 * cpc, 0}
    if cpc > 2:
        ns.add(cpc // 2)
    return sorted(ns)


def make_bits(pattern: str, nsums: int, cpc: int, seed: int = 0) -> np.ndarray:
    """The pattern as nsums bits (u8 0/1)."""
    b = np.zeros(nsums, np.uint8)
    starts = np.arange(0, nsums, cpc)
    ends = np.minimum(starts + cpc, nsums) - 1
    rng = np.random.default_rng(seed * 7919 + nsums * 31 + cpc)
    if pattern == "ones":
        b[:] = 1
    elif pattern == "first":
        b[starts] = 1
    elif pattern == "last":
        b[ends] = 1
    elif pattern == "neighbours":
        # every odd cell is empty; the even cells are full: an odd cell sees set
        # bits only in the words it shares with its neighbours
        for i, (s, e) in enumerate(zip(starts, ends)):
            if i % 2 == 0:
                b[s:e + 1] = 1
    elif pattern == "half":
        b[:] = rng.integers(0, 2, nsums, dtype=np.uint8)
    elif pattern == "sparse":
        b[:] = rng.random(nsums) < 1e-3
    elif pattern != "empty":
        raise ValueError(pattern)
    return b


def pack(bits: np.ndarray) -> np.ndarray:
    """Bits -> u32 words (bit k = bit k % 32 of word k // 32); every bit of the
    last word at or past len(bits) is SET."""
    n = bits.size
    nw = -(-n // 32)
    padded = np.ones(nw * 32, np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def oracle_verdicts(words: np.ndarray, nsums: int, cpc: int) -> np.ndarray:
    """(ncells, 4) u32: count, first, last, 0 -- from np.unpackbits."""
    bits = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:nsums]
    ncells = -(-nsums // cpc) if cpc else 0
    out = np.zeros((ncells, 4), np.uint32)
    for i in range(ncells):
        nz = np.flatnonzero(bits[i * cpc:min((i + 1) * cpc, nsums)])
        out[i] = (nz.size, nz[0] if nz.size else NONE, nz[-1] if nz.size else NONE, 0)
    return out


def as_rows(v: np.ndarray) -> np.ndarray:
    return np.stack([v["mismatches"], v["first_bad"], v["last_bad"], v["reserved"]], axis=1) if v.size \
        else np.zeros((0, 4), np.uint32)


def host_verdicts(hdfs, words, nsums, cpc):
    """The host twin into an array between two guard records; returns the rows."""
    ncells = hdfs.md5_nblocks(nsums, cpc)
    buf = np.full(4 * (ncells + 2), GUARD, np.uint32).view(hdfs.BLOCK_VERDICT_DTYPE)
    rc = hdfs.lib().crc32c_bitmap_verdicts_host(ctypes.c_void_p(words.ctypes.data) if words.size else None, nsums, cpc,
                                                ctypes.c_void_p(buf.ctypes.data + 16))
    assert rc == 0, hdfs.lib().crc32c_last_error()
    raw = buf.view(np.uint32)
    assert (raw[:4] == GUARD).all() and (raw[4 * (ncells + 1):] == GUARD).all(), "a guard record was written"
    return as_rows(buf[1:1 + ncells])


@pytest.mark.parametrize("cpc", CELL_SIZES)
def test_host_twin_against_numpy(hdfs, cpc):
    for nsums in nsums_table(cpc):
        for pat in PATTERNS:
            words = pack(make_bits(pat, nsums, cpc))
            assert words.size == -(-nsums // 32)  # exactly the words the call may read
            got = host_verdicts(hdfs, words, nsums, cpc)
            want = oracle_verdicts(words, nsums, cpc)
            assert got.shape == want.shape and (got == want).all(), \
                "cpc %d, nsums %d, %s: cells %s differ" % (cpc, nsums, pat,
                                                         np.flatnonzero((got != want).any(axis=1))[:8].tolist())


def test_patterns_mean_what_they_say():
    """The oracle on hand-made cases (so that a wrong oracle cannot agree with a wrong twin)."""
    w = np.array([0x80000001, 0xFFFFFFFF], np.uint32)
    assert oracle_verdicts(w, 33, 33).tolist() == [[3, 0, 32, 0]]
    assert oracle_verdicts(w, 33, 16).tolist() == [[1, 0, 0, 0], [1, 15, 15, 0], [1, 0, 0, 0]]
    assert oracle_verdicts(np.zeros(1, np.uint32), 5, 2).tolist() == [[0, NONE, NONE, 0]] * 3
    b = make_bits("neighbours", 100, 10)
    assert b[:10].all() and not b[10:20].any() and b[20:30].all()
    assert pack(np.zeros(33, np.uint8)).tolist() == [0, 0xFFFFFFFE]


def test_wrapper_and_ragged_ranges(hdfs):
    """The Python wrapper; a reader's re-fetch range from first_bad / last_bad."""
    bits = np.zeros(1000, np.uint8)
    bits[[258 + 7, 258 + 200, 999]] = 1
    v = hdfs.bitmap_verdicts_host(pack(bits), 1000, 258)
    assert v.dtype == hdfs.BLOCK_VERDICT_DTYPE and v.size == 4
    assert as_rows(v).tolist() == [[0, NONE, NONE, 0], [2, 7, 200, 0], [0, NONE, NONE, 0], [1, 225, 225, 0]]
    bpc = 512
    assert (int(v[1]["first_bad"]) * bpc, (int(v[1]["last_bad"]) + 1) * bpc) == (3584, 102912)
    assert hdfs.bitmap_verdicts_host(np.zeros(0, np.uint32), 0, 16).size == 0


def test_einval_table(hdfs):
    L = hdfs.lib()
    words = np.zeros(4, np.uint32)
    out = np.full(4 * 8, GUARD, np.uint32)
    w, o = words.ctypes.data, out.ctypes.data
    vp = ctypes.c_void_p
    refused = [
        ("crc_per_cell 0", (vp(w), 64, 0, vp(o))),
        ("NULL bitmap", (None, 64, 16, vp(o))),
        ("NULL verdicts", (vp(w), 64, 16, None)),
        ("bitmap off 4-byte alignment", (vp(w + 2), 64, 16, vp(o))),
        ("verdicts off 4-byte alignment", (vp(w), 64, 16, vp(o + 1))),
    ]
    for what, args in refused:
        assert L.crc32c_bitmap_verdicts_host(*args) == -errno.EINVAL, what
        assert L.crc32c_last_error(), what
        assert (out == GUARD).all(), what
    # nsums == 0: 0 and nothing written, whatever the rest
    assert L.crc32c_bitmap_verdicts_host(None, 0, 0, None) == 0
    assert L.crc32c_bitmap_verdicts_host(vp(w), 0, 16, vp(o)) == 0
    assert (out == GUARD).all()
    # the device call refuses a NULL context before anything else
    assert L.crc32c_bitmap_verdicts(None, vp(w), 64, 16, vp(o), None) == -errno.EINVAL
    assert L.crc32c_plan_verify_blocks(None, None, None, 1, None, None, None) == -errno.EINVAL
    assert L.crc32c_plan_verify_blocks_work_bytes(None, 5) == 0


def test_geometry_hook(hdfs):
    g = hdfs.debug_verdict_geometry()
    assert g["lanes"] == 64
    assert 1 <= g["waves_per_workgroup"] <= 16
    assert 32 <= g["lane_max_cell"] <= 4096
    assert 1 <= g["grid_cap"] <= 65535
    with open(os.path.join(ROOT, "include", "hdfs_crc32c_debug.h")) as f:
        head = f.read().partition("/* ---- 2. libhdfs_crc32c_debug.so only ---- */")[0]
    assert "crc32c_debug_verdict_geometry" in head  # section 1: the product library's


SAN_MAIN = r"""
// Drives crc32c_bitmap_verdicts_host over the size table with every bitmap
// and every output in an exactly-sized heap block, against a bit-by-bit loop.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "hdfs_crc32c.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int main() {
    const uint32_t cells[] = {CELLS};
    long checked = 0;
    for (uint32_t cpc : cells) {
        const uint64_t sizes[] = {3ull * cpc + 1, 2ull * cpc + (cpc > 1 ? cpc - 1 : 1), cpc > 1 ? cpc - 1 : 1, 4ull * cpc,
                                  cpc / 2};
        for (uint64_t nsums : sizes) {
            if (!nsums) continue;
            for (int pat = 0; pat < 4; ++pat) {
                const uint64_t nw = (nsums + 31) / 32, nc = (nsums + cpc - 1) / cpc;
                uint32_t *bits = static_cast<uint32_t *>(malloc(nw * 4));  // exactly the words the call may read
                for (uint64_t w = 0; w < nw; ++w)
                    bits[w] = pat == 0 ? 0u : pat == 1 ? 0xffffffffu : pat == 2 ? uint32_t(rnd())
                                                                               : uint32_t(rnd() & rnd() & rnd() & rnd());
                crc32c_block_verdict *v = static_cast<crc32c_block_verdict *>(malloc(nc * sizeof *v));
                if (crc32c_bitmap_verdicts_host(bits, nsums, cpc, v) != 0) return 3;
                for (uint64_t c = 0; c < nc; ++c) {
                    uint32_t n = 0, lo = 0xffffffffu, hi = 0xffffffffu;
                    for (uint64_t k = c * cpc; k < (c + 1) * cpc && k < nsums; ++k)
                        if ((bits[k / 32] >> (k % 32)) & 1u) {
                            if (!n++) lo = uint32_t(k - c * cpc);
                            hi = uint32_t(k - c * cpc);
                        }
                    if (v[c].mismatches != n || v[c].first_bad != lo || v[c].last_bad != hi || v[c].reserved) {
                        printf("cpc %u nsums %llu pat %d cell %llu differs\n", cpc, (unsigned long long)nsums, pat,
                               (unsigned long long)c);
                        return 1;
                    }
                    ++checked;
                }
                free(v);
                free(bits);
            }
        }
    }
    if (crc32c_bitmap_verdicts_host(nullptr, 0, 0, nullptr) != 0) return 4;
    if (crc32c_bitmap_verdicts_host(nullptr, 5, 1, nullptr) == 0) return 5;
    printf("verdict sanitizer run clean: %ld cells\n", checked);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_twin_under_asan_ubsan(tmp_path):
    """The host twin (and the word arithmetic it shares with the kernel,
    csrc/verdict_cell.h) as a stand-alone AddressSanitizer + UBSan program:
    shifts by 32 and masks at word edges are where this code goes wrong."""
    csrc = os.path.join(ROOT, "native-hdfs-fuse_amd", "csrc")
    main = tmp_path / "verdicts_main.cpp"
    main.write_text(SAN_MAIN.replace("CELLS", ", ".join(str(c) for c in CELL_SIZES)))
    exe = str(tmp_path / "verdicts_san")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, str(main),
                    os.path.join(csrc, "verdicts_host.cpp"), os.path.join(csrc, "errors.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verdict sanitizer run clean" in r.stdout
