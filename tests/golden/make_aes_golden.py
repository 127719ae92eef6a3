#!/usr/bin/env python3
"""Regenerate tests/golden/aes_ctr.json from OpenSSL (the ``openssl enc``
command line; none of this library's code takes part).

The fixture holds NIST SP 800-38A F.5 known answers and counter-carry
keystream blocks (each recomputed with OpenSSL here and compared with the
published values), and per key size the SHA-256 of the ciphertext of 1 MiB of
the documented xorshift64 stream (``oracle.xorshift64_bytes``, the project's
seed) at stream offset 2^40 + 5.

A stream offset s is given to OpenSSL as IV = IV + (s >> 4) (128-bit
big-endian) with s % 16 dummy bytes in front of the data, which are dropped
from the output again.

Run from the repo root:  python tests/golden/make_aes_golden.py
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "aes_ctr.json")

NIST_IV = "f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff"
NIST_PLAIN = "6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
NIST = [  # (key, ciphertext prefix) -- SP 800-38A F.5.1, F.5.3, F.5.5
    ("2b7e151628aed2a6abf7158809cf4f3c", "874d6191b620e3261bef6864990db6ce9806f66b7970fdff8617187bb9fffdff"),
    ("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b", "1abc932417521ca24f2b0459fe7e6e0b"),
    ("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4", "601ec313775789a5b7a7f504bbf3d228"),
]
CARRY = [  # (iv, keystream block 1 under the 128-bit NIST key)
    ("0000000000000000ffffffffffffffff", "dc0a3bc38609c26f6f2a63a39cf7ee93"),
    ("ffffffffffffffffffffffffffffffff", "7df76b0c1ab899b33e42f047b91b546f"),
]
GOLDEN_IV = "000102030405060708090a0b0c0d0e0f"
GOLDEN_OFF = (1 << 40) + 5
GOLDEN_BYTES = 1 << 20


def openssl_ctr(key_hex: str, iv_hex: str, stream_off: int, data: bytes) -> bytes:
    iv = (int(iv_hex, 16) + (stream_off >> 4)) % (1 << 128)
    pad = stream_off & 15
    r = subprocess.run(["openssl", "enc", "-aes-%d-ctr" % (4 * len(key_hex)), "-nopad", "-K", key_hex, "-iv",
                        "%032x" % iv], input=bytes(pad) + data, capture_output=True, check=True)
    assert len(r.stdout) == pad + len(data)
    return r.stdout[pad:]


def main() -> None:
    plain = bytes.fromhex(NIST_PLAIN)
    known = []
    for key, want in NIST:
        got = openssl_ctr(key, NIST_IV, 0, plain).hex()
        assert got.startswith(want), (key, got)
        known.append({"key": key, "iv": NIST_IV, "plaintext": NIST_PLAIN, "ciphertext": got})
    carry = []
    for iv, want in CARRY:
        got = openssl_ctr(NIST[0][0], iv, 16, bytes(16)).hex()
        assert got == want, (iv, got)
        carry.append({"key": NIST[0][0], "iv": iv, "keystream_block_1": got})
    data = oracle.xorshift64_bytes(GOLDEN_BYTES, oracle.SEED).tobytes()
    golden = []
    for bits in (128, 192, 256):
        key = bytes(range(0x10, 0x10 + bits // 8)).hex()
        ct = openssl_ctr(key, GOLDEN_IV, GOLDEN_OFF, data)
        golden.append({"key": key, "iv": GOLDEN_IV, "stream_off": GOLDEN_OFF, "bytes": GOLDEN_BYTES,
                       "fill": "xorshift", "seed": oracle.SEED, "sha256": hashlib.sha256(ct).hexdigest()})
    ver = subprocess.run(["openssl", "version"], capture_output=True, text=True, check=True).stdout.strip()
    with open(OUT, "w") as f:
        json.dump({"source": ver, "known_answers": known, "carry": carry, "golden": golden}, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
