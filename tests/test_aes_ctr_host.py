"""AES/CTR/NoPadding on the host (include/hdfs_crc32c.h section 7;
csrc/aes_ctr.h, csrc/aes_ctr_host.cpp): hdfs_aes_ctr_init, hdfs_aes_ctr_counter,
hdfs_aes_ctr_xor and hdfs_aes_wire_segments.  Expected bytes: NIST SP 800-38A
F.5, the ``openssl enc`` command line on random cases (skipped only where
there is no ``openssl``), and goldens OpenSSL wrote
(tests/golden/make_aes_golden.py -> tests/golden/aes_ctr.json), which never
skip.  No GPU."""
from __future__ import annotations

import ctypes
import errno
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "aes_ctr.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def megabyte():
    d = oracle.xorshift64_bytes(1 << 20, oracle.SEED)
    d.setflags(write=False)
    return d


def _aes(hdfs, key_hex, iv_hex):
    return hdfs.AesCtr(bytes.fromhex(key_hex), bytes.fromhex(iv_hex))


# ---- known answers ---------------------------------------------------------------
def test_nist_sp800_38a_f5(hdfs, fixture):
    """F.5.1 (all of it), F.5.3 and F.5.5 (the published first block, the rest as OpenSSL gives it)."""
    published = {16: "874d6191b620e3261bef6864990db6ce9806f66b7970fdff8617187bb9fffdff",
                 24: "1abc932417521ca24f2b0459fe7e6e0b", 32: "601ec313775789a5b7a7f504bbf3d228"}
    assert len(fixture["known_answers"]) == 3
    for ka in fixture["known_answers"]:
        aes = _aes(hdfs, ka["key"], ka["iv"])
        assert aes.rounds == {16: 10, 24: 12, 32: 14}[len(ka["key"]) // 2]
        got = aes.xor(0, bytes.fromhex(ka["plaintext"])).tobytes().hex()
        assert got == ka["ciphertext"]
        assert got.startswith(published[len(ka["key"]) // 2])
        # decrypting is the same call
        assert aes.xor(0, bytes.fromhex(got)).tobytes().hex() == ka["plaintext"]


def test_counter_carry(hdfs, fixture):
    """Keystream block 1 when the carry enters the high half, and when the counter wraps to 0."""
    published = {"0000000000000000ffffffffffffffff": "dc0a3bc38609c26f6f2a63a39cf7ee93",
                 "ff" * 16: "7df76b0c1ab899b33e42f047b91b546f"}
    assert {c["iv"] for c in fixture["carry"]} == set(published)
    for c in fixture["carry"]:
        assert c["keystream_block_1"] == published[c["iv"]]
        assert _aes(hdfs, c["key"], c["iv"]).xor(16, bytes(16)).tobytes().hex() == published[c["iv"]]
    ctr = hdfs.AesCtr.counter
    assert ctr(bytes.fromhex("0000000000000000ffffffffffffffff"), 1).hex() == "0000000000000001" + "00" * 8
    assert ctr(b"\xff" * 16, 1) == bytes(16)
    assert ctr(b"\xff" * 16, 0) == b"\xff" * 16
    assert ctr(bytes(15) + b"\x01", (1 << 64) - 1).hex() == "0000000000000001" + "00" * 8
    rng = np.random.default_rng(7)
    for _ in range(200):
        iv = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        n = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        assert int.from_bytes(ctr(iv, n), "big") == (int.from_bytes(iv, "big") + n) % (1 << 128)


def test_init_errors(hdfs):
    for nbytes in (0, 8, 15, 17, 20, 31, 33, 64):
        with pytest.raises(hdfs.Crc32cError) as e:
            hdfs.AesCtr(bytes(range(nbytes)), bytes(16))
        assert e.value.rc == -errno.EINVAL
        if nbytes >= 8:  # key bytes never appear in an error text
            assert bytes(range(nbytes)).hex()[:16] not in str(e.value)
    L = hdfs.lib()
    c = (ctypes.c_uint8 * 272)()
    buf = (ctypes.c_uint8 * 32)()
    assert L.hdfs_aes_ctr_init(None, buf, 128, buf) == -errno.EINVAL
    assert L.hdfs_aes_ctr_init(c, None, 128, buf) == -errno.EINVAL
    assert L.hdfs_aes_ctr_init(c, buf, 128, None) == -errno.EINVAL
    # xor: bad rounds, NULL with bytes, an offset past 2^64; length 0 is fine even with NULL
    aes = hdfs.AesCtr(bytes(16), bytes(16))
    assert L.hdfs_aes_ctr_xor(aes.handle, 0, None, None, 0) == 0
    assert L.hdfs_aes_ctr_xor(aes.handle, 0, None, buf, 16) == -errno.EINVAL
    assert L.hdfs_aes_ctr_xor(aes.handle, 0, buf, None, 16) == -errno.EINVAL
    assert L.hdfs_aes_ctr_xor(None, 0, buf, buf, 16) == -errno.EINVAL
    assert L.hdfs_aes_ctr_xor(aes.handle, (1 << 64) - 8, buf, buf, 16) == -errno.EINVAL
    assert L.hdfs_aes_ctr_xor(aes.handle, (1 << 64) - 16, buf, buf, 16) == 0  # ends exactly at 2^64
    aes.c.rounds = 11
    assert L.hdfs_aes_ctr_xor(aes.handle, 0, buf, buf, 16) == -errno.EINVAL
    # without a context the device forms say -ENODEV where there is no GPU, else -EINVAL
    want = -errno.ENODEV if hdfs.device_count() == 0 else -errno.EINVAL
    assert L.hdfs_aes_ctr_xor_strided_dev(None, aes.handle, buf, buf, 16, 1, 0, 0, 0, 0, None) == want
    assert L.hdfs_aes_ctr_xor_list_dev(None, aes.handle, None, 0, None) == want


# ---- against the openssl command line --------------------------------------------------
def _openssl(key: bytes, iv: bytes, data: bytes) -> bytes:
    r = subprocess.run(["openssl", "enc", "-aes-%d-ctr" % (8 * len(key)), "-nopad", "-K", key.hex(), "-iv", iv.hex()],
                       input=data, capture_output=True, check=True)
    return r.stdout


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl command line")
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_random_cases_against_openssl(hdfs, bits):
    """Random keys, IVs, lengths and stream offsets: a stream offset s reaches OpenSSL as
    IV = hdfs_aes_ctr_counter(iv, s / 16) with s % 16 dummy bytes in front (which also pins
    counter)."""
    rng = np.random.default_rng(bits)
    for case in range(12):
        key = rng.integers(0, 256, bits // 8, dtype=np.uint8).tobytes()
        iv = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        if case % 4 == 1:
            iv = iv[:8] + b"\xff" * 7 + iv[15:]  # a carry into the high half within the data
        if case % 4 == 2:
            iv = b"\xff" * 15 + iv[15:]          # the counter wraps
        n = int(rng.integers(0, 5000))
        s = int(rng.integers(0, 1 << 50)) if case % 3 else int(rng.integers(0, 64))
        data = rng.integers(0, 256, n, dtype=np.uint8)
        pad = s % 16
        want = _openssl(key, hdfs.AesCtr.counter(iv, s // 16), bytes(pad) + data.tobytes())[pad:]
        assert hdfs.AesCtr(key, iv).xor(s, data).tobytes() == want, (case, n, s)


# ---- goldens (never skip) -----------------------------------------------------------------
def test_goldens(hdfs, fixture, megabyte):
    assert [len(g["key"]) * 4 for g in fixture["golden"]] == [128, 192, 256]
    for g in fixture["golden"]:
        assert (g["bytes"], g["seed"], g["stream_off"]) == (megabyte.size, oracle.SEED, (1 << 40) + 5)
        ct = _aes(hdfs, g["key"], g["iv"]).xor(g["stream_off"], megabyte)
        assert hashlib.sha256(ct.tobytes()).hexdigest() == g["sha256"]


# ---- split invariance, alignment, in place ----------------------------------------------------
def test_split_invariance(hdfs, megabyte):
    """xor(s, A || B) == xor(s, A) || xor(s + |A|, B) over random cuts and offsets."""
    rng = np.random.default_rng(11)
    aes = hdfs.AesCtr(bytes(range(32)), bytes(range(16)))
    for _ in range(60):
        n = int(rng.integers(1, 3000))
        s = int(rng.integers(0, 1 << 45))
        data = megabyte[:n]
        whole = aes.xor(s, data)
        cuts = sorted(set(int(x) for x in rng.integers(0, n + 1, 4)) | {0, n})
        parts = [aes.xor(s + a, data[a:b]) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts), whole)
    assert aes.xor(5, b"").size == 0


def test_every_host_alignment_and_in_place(hdfs, megabyte):
    aes = hdfs.AesCtr(bytes(range(24)), bytes(range(16)))
    n = 1000
    for a_in in range(16):
        for a_out in range(16):
            s = 7 * a_in + a_out
            src = np.zeros(n + 32, np.uint8)
            base = (-src.ctypes.data) % 16
            view = src[base + a_in:base + a_in + n]
            view[:] = megabyte[100:100 + n]
            dst = np.full(n + 48, 0xEE, np.uint8)
            obase = (-dst.ctypes.data) % 16 + 16
            out = dst[obase + a_out:obase + a_out + n]
            assert (view.ctypes.data % 16, out.ctypes.data % 16) == (a_in, a_out)
            aes.xor(s, view, out)
            want = aes.xor(s, megabyte[100:100 + n])
            assert np.array_equal(out, want)
            assert (dst[:obase + a_out] == 0xEE).all() and (dst[obase + a_out + n:] == 0xEE).all()
        aes.xor(s, view, view)  # in place
        assert np.array_equal(view, want)


# ---- the wire layout -------------------------------------------------------------------------------
def test_wire_segments(hdfs, orc, megabyte):
    """A batch's whole wire image (prefixes from crc32c_frame_packets + data; a ragged last packet and
    the empty final one) encrypted as ONE stream equals the prefixes and the data segments encrypted one
    by one at the offsets hdfs_aes_wire_segments reports."""
    bpc = 512
    lens = [65536, 65536, 1000, 0]
    rows, pos, idx = [], 0, 0
    for n in lens:
        rows.append((pos, idx, n, bpc))
        pos += n
        idx += -(-n // bpc)
    pk = np.array(rows, dtype=hdfs.PACKET_DTYPE)
    payload = megabyte[:pos]
    sums = orc.batch(payload, pk, idx)
    prefixes, offs = hdfs.frame_packets(pk, sums)
    wire = b"".join(prefixes[int(offs[i]):int(offs[i + 1])] + payload[r[0]:r[0] + r[2]].tobytes()
                    for i, r in enumerate(rows))
    base = (1 << 33) + 11
    aes = hdfs.AesCtr(bytes(range(16)), bytes(range(16, 32)))
    whole = aes.xor(base, wire).tobytes()
    pre_off, segs = hdfs.aes_wire_segments(pk, offs, base, 1 << 20, 1 << 21)
    assert len(pre_off) == len(segs) == len(rows)
    pieces, at = [], base
    for i, r in enumerate(rows):
        p = prefixes[int(offs[i]):int(offs[i + 1])]
        assert int(pre_off[i]) == at
        pieces.append(aes.xor(int(pre_off[i]), p).tobytes())
        at += len(p)
        assert (int(segs[i]["src"]), int(segs[i]["dst"])) == ((1 << 20) + r[0], (1 << 21) + r[0])
        assert (int(segs[i]["stream_off"]), int(segs[i]["len"])) == (at, r[2])
        pieces.append(aes.xor(at, payload[r[0]:r[0] + r[2]]).tobytes())
        at += r[2]
    assert b"".join(pieces) == whole
    assert at == base + len(wire)
    # too little room, an empty batch
    L = hdfs.lib()
    o = np.ascontiguousarray(offs, np.uint64)
    seg = np.zeros(4, hdfs.AES_SEGMENT_DTYPE)
    pre = np.zeros(4, np.uint64)
    assert L.hdfs_aes_wire_segments(pk.ctypes.data, 4, o.ctypes.data, 0, None, None, seg.ctypes.data, pre.ctypes.data,
                                    3) == -errno.EINVAL
    assert L.hdfs_aes_wire_segments(None, 0, None, 0, None, None, None, None, 0) == 0
