"""Erasure coding on the host (include/hdfs_crc32c.h section 8;
csrc/ec_gf256.h, csrc/ec_host.cpp): the field, the encode and decode matrices,
hdfs_ec_apply, the striped layout and the packets of a data block over the
file-order buffer.  Expected values: tests/golden/ec_rs.json and the bitwise
multiply of its generator tests/golden/make_ec_golden.py, an independent
pure-Python implementation that shares no table with the library.  CPU only;
all results are bit-exact."""
from __future__ import annotations

import ctypes
import errno
import hashlib
import importlib.util
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

SCHEMES = [("rs", 6, 3), ("rs", 3, 2), ("rs", 10, 4), ("xor", 2, 1)]


@pytest.fixture(scope="module")
def ref():
    """The golden generator as a module (its bitwise mul / inv / matrices)."""
    spec = importlib.util.spec_from_file_location("make_ec_golden", os.path.join(GOLDEN, "make_ec_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ec_rs.json")) as f:
        return json.load(f)


def codec_of(hdfs, name):
    return hdfs.EC_XOR if name == "xor" else hdfs.EC_RS


def pin_units(k, n):
    t = np.arange(n, dtype=np.int64)
    return [((31 * j + 7 * t + 1) & 0xff).astype(np.uint8) for j in range(k)]


# ---- the field ------------------------------------------------------------------------
def test_generator_reproduces_the_pins(ref):
    ref.check_pins()


def test_field_all_products(hdfs, ref):
    L = hdfs.lib()
    got = np.array([[L.hdfs_gf256_mul(a, b) for b in range(256)] for a in range(256)], np.uint8)
    want = np.array([[ref.mul(a, b) for b in range(256)] for a in range(256)], np.uint8)
    assert np.array_equal(got, want)
    assert (got[0x53, 0xca], got[2, 0x80]) == (0x8f, 0x1d)
    # the axioms, over the library's own table: commutative, 1 neutral, 0 absorbing, no zero
    # divisors, associative and distributive over xor (all triples of a sample of the field)
    assert np.array_equal(got, got.T) and np.array_equal(got[1], np.arange(256)) and not got[0].any()
    assert (got[1:, 1:] != 0).all()
    s = np.array([1, 2, 3, 0x1d, 0x53, 0x80, 0x8e, 0xca, 0xf4, 0xff])
    for a in s:
        for b in s:
            assert np.array_equal(got[got[a, b], :], got[a, got[b, :]])
            assert np.array_equal(got[a, b ^ np.arange(256)], got[a, b] ^ got[a, :])


def test_field_inverses(hdfs, golden):
    inv = [hdfs.gf256_inv(a) for a in range(256)]
    assert bytes(inv).hex() == golden["field"]["inv"]
    assert (inv[0], inv[1], inv[2], inv[3]) == (0, 1, 0x8e, 0xf4)
    assert all(hdfs.gf256_mul(a, inv[a]) == 1 for a in range(1, 256))
    for a, b, c in golden["field"]["mul"]:
        assert hdfs.gf256_mul(a, b) == c


# ---- the matrices and the parity pins ------------------------------------------------------
@pytest.mark.parametrize("codec,k,m", SCHEMES)
def test_encode_matrix_and_parity_pins(hdfs, golden, codec, k, m):
    g = next(s for s in golden["schemes"] if (s["codec"], s["k"], s["m"]) == (codec, k, m))
    mx = hdfs.EcMatrix.encode(k, m, codec_of(hdfs, codec))
    assert (mx.n_in, mx.n_out) == (k, m)
    assert [bytes(r).hex() for r in mx.rows] == g["parity_matrix"]
    par = mx.apply(pin_units(k, g["unit_bytes"]))
    assert [p[:16].tobytes().hex() for p in par] == g["parity_first16"]
    assert hashlib.sha256(b"".join(p.tobytes() for p in par)).hexdigest() == g["parity_sha256"]


def test_stated_pins(hdfs):
    """The values stated with the feature, spelled out here as well."""
    rows = [bytes(r).hex() for r in hdfs.EcMatrix.encode(6, 3).rows]
    assert rows == ["7aba47a78ef4", "ba7aa747f48e", "ad9ddd983daa"]
    assert [bytes(r).hex() for r in hdfs.EcMatrix.encode(3, 2).rows] == ["f48e01", "47a77a"]
    assert bytes(hdfs.EcMatrix.encode(10, 4).rows[3]).hex() == "aa3d965d9dad98dda747"
    par = hdfs.EcMatrix.encode(6, 3).apply(pin_units(6, 4096))
    assert par[0][:16].tobytes().hex() == "127eb5a56ffa1909909005dcdf764c8c"
    assert par[2][:16].tobytes().hex() == "495c1c224a9e69132d8140f81611c834"
    assert hashlib.sha256(b"".join(p.tobytes() for p in par)).hexdigest() == \
        "d63542f1fd97d85fe9158c1909ef608d684100d7c5859687d09b5643050dd1c6"
    assert hdfs.EcMatrix.encode(10, 4).apply(pin_units(10, 16))[0].tobytes().hex() == "d65309429c5a9f8f5b0f83384843ae51"


@pytest.mark.parametrize("codec,k,m", SCHEMES)
def test_every_erasure_pattern_round_trips(hdfs, golden, codec, k, m):
    """Every pattern of 1 .. m lost units, decoded from the first k survivors and from the last k,
    restores the data and the parity exactly; the decode matrices of all m-unit patterns (first k
    survivors) have the generator's digest, and the listed ones equal the generator's."""
    g = next(s for s in golden["schemes"] if (s["codec"], s["k"], s["m"]) == (codec, k, m))
    listed = {tuple(p["erased"]): p for p in g["decode"]}
    c = codec_of(hdfs, codec)
    rng = np.random.default_rng(k * 16 + m)
    data = [rng.integers(0, 256, 67, dtype=np.uint8) for _ in range(k)]
    units = data + hdfs.EcMatrix.encode(k, m, c).apply(data)
    digest, seen, found = hashlib.sha256(), 0, 0
    for n in range(1, m + 1):
        for erased in itertools.combinations(range(k + m), n):
            alive = [u for u in range(k + m) if u not in erased]
            for valid in ([alive[:k]] if n == m else [alive[:k], alive[-k:]]):  # (n == m: the same k)
                dec = hdfs.EcMatrix.decode(k, m, valid, erased, c)
                assert (dec.n_in, dec.n_out) == (k, n)
                back = dec.apply([units[v] for v in valid])
                for e, b in zip(erased, back):
                    assert np.array_equal(b, units[e]), (erased, valid, e)
                if n == m:
                    digest.update(bytes(erased) + b"".join(bytes(r) for r in dec.rows))
                    seen += 1
                    if erased in listed:
                        assert listed[erased]["valid"] == valid
                        assert [bytes(r).hex() for r in dec.rows] == listed[erased]["rows"]
                        found += 1
    assert seen == g["decode_patterns"] and found == len(g["decode"])
    assert digest.hexdigest() == g["decode_sha256"]


def test_decode_orders_follow_the_lists(hdfs):
    """Columns come in the order of `valid`, rows in the order of `erased`."""
    a = hdfs.EcMatrix.decode(6, 3, [0, 2, 3, 5, 6, 8], [1, 4, 7]).rows
    b = hdfs.EcMatrix.decode(6, 3, [8, 2, 3, 5, 6, 0], [7, 1, 4]).rows
    perm = [5, 1, 2, 3, 4, 0]
    assert b == [[a[r][perm[i]] for i in range(6)] for r in (2, 0, 1)]


# ---- hdfs_ec_apply ------------------------------------------------------------------------------
@pytest.mark.parametrize("absent", [[0], [2], [5], [0, 5], [0, 1, 2, 3, 4, 5]])
def test_null_inputs_are_zeros(hdfs, absent):
    mx = hdfs.EcMatrix.encode(6, 3)
    rng = np.random.default_rng(7)
    data = [rng.integers(0, 256, 301, dtype=np.uint8) for _ in range(6)]
    zeroed = [np.zeros(301, np.uint8) if j in absent else d for j, d in enumerate(data)]
    want = mx.apply(zeroed)
    outs = [np.full(301 + 32, 0xEE, np.uint8) for _ in range(3)]
    mx.apply_ptrs([None if j in absent else d.ctypes.data for j, d in enumerate(data)],
                  [o.ctypes.data + 16 for o in outs], 301)
    for o, w in zip(outs, want):
        assert np.array_equal(o[16:-16], w) and (o[:16] == 0xEE).all() and (o[-16:] == 0xEE).all()


def test_apply_any_alignment_and_shape(hdfs, ref):
    """n_in x n_out shapes of arbitrary coefficients at odd addresses against the bitwise reference;
    nothing outside [out, out + len) is written."""
    rng = np.random.default_rng(11)
    for n_in, n_out, n in [(1, 1, 1), (3, 2, 255), (16, 4, 257), (10, 4, 513), (6, 3, 16)]:
        rows = rng.integers(0, 256, (n_out, n_in)).tolist()
        mx = hdfs.EcMatrix(rows)
        ins = [rng.integers(0, 256, n + 32, dtype=np.uint8) for _ in range(n_in)]
        outs = [np.full(n + 64, 0xEE, np.uint8) for _ in range(n_out)]
        offs_in = [(3 * j + 1) % 16 for j in range(n_in)]
        offs_out = [16 + (5 * r + 2) % 16 for r in range(n_out)]
        mx.apply_ptrs([a.ctypes.data + o for a, o in zip(ins, offs_in)],
                      [a.ctypes.data + o for a, o in zip(outs, offs_out)], n)
        want = ref.apply(rows, [a[o:o + n].tobytes() for a, o in zip(ins, offs_in)])
        for r in range(n_out):
            img = np.full(n + 64, 0xEE, np.uint8)
            img[offs_out[r]:offs_out[r] + n] = np.frombuffer(want[r], np.uint8)
            assert np.array_equal(outs[r], img), (n_in, n_out, r)


# ---- the striped layout ----------------------------------------------------------------------------
def layout_by_cells(length, k, m, cell):
    """StripedBlockUtil's rule cell by cell: cell i belongs to data block i % k."""
    lens = [0] * k
    i = 0
    while i * cell < length:
        lens[i % k] += min(cell, length - i * cell)
        i += 1
    return lens + [lens[0]] * m


@pytest.mark.parametrize("k,m,cell", [(6, 3, 4096), (3, 2, 1024), (10, 4, 512), (2, 1, 65536)])
def test_group_layout(hdfs, k, m, cell):
    for length in (0, 1, cell - 1, cell, cell + 1, k * cell, k * cell + 1, 2 * k * cell + cell // 2):
        got = hdfs.ec_group_layout(length, k, m, cell)
        assert got == layout_by_cells(length, k, m, cell), length
        assert sum(got[:k]) == length


@pytest.mark.parametrize("k,cell,packetsize,bpc", [(6, 4096, 2048, 512), (3, 8192, 8192, 1024), (10, 1024, 512, 128)])
def test_block_packets(hdfs, k, cell, packetsize, bpc):
    """The checksums of a gathered copy of each data block (crc32c_chunks_cpu) equal those of a
    plan-shaped walk of the block's packets over the file-order buffer."""
    rng = np.random.default_rng(k)
    for length in (1, cell, cell + 1, k * cell, k * cell + 1, 2 * k * cell + cell // 2, 3 * k * cell + 2 * cell + 77):
        buf = rng.integers(0, 256, length, dtype=np.uint8)
        lens = hdfs.ec_group_layout(length, k, 1, cell)
        ncells = -(-length // cell)
        for b in range(k):
            gathered = np.concatenate([buf[i * cell:(i + 1) * cell] for i in range(b, ncells, k)] + [np.zeros(0, np.uint8)])
            assert gathered.size == lens[b]
            pk = hdfs.ec_block_packets(length, k, cell, b, packetsize, bpc, out_idx0=5)
            want_lens = [n for n in hdfs.packetize(lens[b], 0, packetsize, bpc) if n]
            assert [int(n) for n in pk["len"]] == want_lens and (pk["bpc"] == bpc).all()
            nsums = hdfs.nchunks(lens[b], bpc) if lens[b] else 0
            got = np.zeros(5 + nsums, np.uint32)
            for p in pk:
                off, n, idx = int(p["payload_off"]), int(p["len"]), int(p["out_idx"])
                assert (off // cell) % k == b and off + n <= length and (off % cell) + n <= cell
                got[idx:idx + hdfs.nchunks(n, bpc)] = hdfs.chunks_cpu(buf[off:off + n], bpc)
            if lens[b]:
                assert np.array_equal(got[5:], hdfs.chunks_cpu(gathered, bpc)), (length, b)
            else:
                assert pk.size == 0


# ---- argument errors -------------------------------------------------------------------------------
def test_argument_errors(hdfs):
    L = hdfs.lib()
    E = -errno.EINVAL
    mx = hdfs.EcMatrix()
    h = mx.handle
    for codec, k, m in [(0, 0, 3), (0, 17, 3), (0, 6, 0), (0, 6, 5), (1, 2, 2), (1, 2, 0), (2, 6, 3), (-1, 6, 3)]:
        assert L.hdfs_ec_encode_matrix(codec, k, m, h) == E, (codec, k, m)
        assert b"hdfs_ec_encode_matrix" in L.crc32c_last_error()
    assert L.hdfs_ec_encode_matrix(0, 6, 3, None) == E
    assert L.hdfs_ec_encode_matrix(0, 16, 4, h) == 0 and L.hdfs_ec_encode_matrix(1, 16, 1, h) == 0

    def dec(valid, erased, k=6, m=3, codec=0, n=None):
        v = np.array(valid, np.uint32)
        e = np.array(erased, np.uint32)
        return L.hdfs_ec_decode_matrix(codec, k, m, v.ctypes.data, e.ctypes.data, len(erased) if n is None else n, h)

    ok = [0, 2, 3, 5, 6, 8]
    assert dec(ok, [1, 4, 7]) == 0
    assert dec([0, 2, 3, 5, 6, 9], [1]) == E          # a valid index out of range
    assert dec(ok, [9]) == E                          # an erased index out of range
    assert dec([0, 2, 3, 5, 6, 6], [1]) == E          # a duplicate among the valid
    assert dec(ok, [1, 1]) == E                       # a duplicate among the erased
    assert dec(ok, [2]) == E                          # an index in both lists
    assert dec(ok, [1], n=0) == E                     # n_erased == 0
    assert dec(list(range(10)), [10, 11, 12, 13, 10], k=10, m=4) == E  # n_erased above 4
    assert dec(ok, [1], k=0) == E and dec(ok, [1], m=5) == E and dec([0, 1], [2], k=2, m=2, codec=1) == E
    assert L.hdfs_ec_decode_matrix(0, 6, 3, None, None, 1, h) == E
    out = np.zeros(20, np.uint64)
    assert L.hdfs_ec_group_layout(100, 6, 3, 0, out.ctypes.data) == E
    assert L.hdfs_ec_group_layout(100, 0, 3, 16, out.ctypes.data) == E
    assert L.hdfs_ec_group_layout(100, 6, 3, 16, None) == E
    bp = L.hdfs_ec_block_packets
    assert bp(1 << 20, 6, 4096, 0, 3000, 500, 0, None, 0) == E   # cell % packetsize
    assert bp(1 << 20, 6, 4096, 0, 2048, 500, 0, None, 0) == E   # packetsize % bpc
    assert bp(1 << 20, 6, 4096, 6, 2048, 512, 0, None, 0) == E   # block >= k
    assert bp(1 << 20, 6, 0, 0, 2048, 512, 0, None, 0) == E and bp(1 << 20, 6, 4096, 0, 2048, 0, 0, None, 0) == E
    pk = np.zeros(4, hdfs.PACKET_DTYPE)
    assert bp(1 << 20, 6, 4096, 0, 2048, 512, 0, pk.ctypes.data, 4) == E  # room for 4 of many
    assert bp(1 << 20, 6, 4096, 0, 2048, 512, 0, None, 0) > 4
    # hdfs_ec_apply: a bad matrix, NULL arrays and outputs, overlaps; len == 0 is fine
    good = hdfs.EcMatrix.encode(3, 2)
    a = np.zeros(256, np.uint8)
    p = a.ctypes.data
    bad = hdfs.EcMatrix.encode(3, 2)
    for n_in, n_out in [(0, 2), (17, 2), (3, 0), (3, 5)]:
        bad.c.n_in, bad.c.n_out = n_in, n_out
        with pytest.raises(hdfs.Crc32cError) as e:
            bad.apply_ptrs([p] * n_in, [p + 128] * n_out, 16)
        assert e.value.rc == E
    refused = [
        lambda: good.apply_ptrs([p, p + 16, p + 32], [p + 64, 0], 16),           # a NULL output
        lambda: good.apply_ptrs([p, p + 16, p + 32], [p + 40, p + 64], 16),      # an output over an input
        lambda: good.apply_ptrs([p, p + 16, p + 32], [p + 64, p + 70], 16),      # an output over an output
        lambda: good.apply_ptrs(None, [p + 64, p + 96], 16),
    ]
    for call in refused:
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == E
    assert L.hdfs_ec_apply(None, None, None, 16) == E
    good.apply_ptrs(None, None, 0)
    good.apply_ptrs([0, 0, 0], [p, p + 16], 16)  # all-NULL inputs: zeros
    assert not a.any()
    assert ctypes.sizeof(hdfs._EcMatrixStruct) == 80
    # without a context the device forms say -ENODEV where there is no GPU, else -EINVAL
    want = -errno.ENODEV if hdfs.device_count() == 0 else E
    ins = (ctypes.c_void_p * 3)(p, p + 16, p + 32)
    outs = (ctypes.c_void_p * 2)(p + 64, p + 96)
    assert L.hdfs_ec_apply_dev(None, good.handle, ins, outs, 16, None) == want
    assert L.hdfs_ec_encode_striped_dev(None, good.handle, p, 48, 16, outs, None) == want
