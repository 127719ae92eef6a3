"""Generates tests/golden/ec_rs.json: an independent, pure-Python, bitwise
implementation of the erasure-coding arithmetic of include/hdfs_crc32c.h
section 8 -- GF(2^8) mod x^8+x^4+x^3+x^2+1 (0x11d) by shift-and-xor, inverses by
search, the Cauchy parity matrix P[r][j] = inv((k + r) ^ j), decode matrices by
Gauss-Jordan elimination.  It shares no table and no code with the library.

The pins stated with the feature (products, inverses, the rows of P, the first
16 parity bytes and the SHA-256 of the parity of 4096-byte units, data unit j
byte t = (31 j + 7 t + 1) & 0xff) are asserted here before anything is written.

    python tests/golden/make_ec_golden.py
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMES = [("rs", 6, 3), ("rs", 3, 2), ("rs", 10, 4), ("xor", 2, 1)]


def mul(a: int, b: int) -> int:
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11d
        b >>= 1
    return r


def inv(a: int) -> int:
    if a == 0:
        return 0
    return next(x for x in range(1, 256) if mul(a, x) == 1)


def parity_matrix(codec: str, k: int, m: int):
    if codec == "xor":
        return [[1] * k]
    return [[inv((k + r) ^ j) for j in range(k)] for r in range(m)]


def generator(codec: str, k: int, m: int):
    return [[int(i == j) for j in range(k)] for i in range(k)] + parity_matrix(codec, k, m)


def invert(a):
    n = len(a)
    a = [row[:] + [int(i == j) for j in range(n)] for i, row in enumerate(a)]
    for c in range(n):
        p = next(r for r in range(c, n) if a[r][c])
        a[c], a[p] = a[p], a[c]
        d = inv(a[c][c])
        a[c] = [mul(v, d) for v in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [v ^ mul(f, w) for v, w in zip(a[r], a[c])]
    return [row[n:] for row in a]


def decode_matrix(codec: str, k: int, m: int, valid, erased):
    g = generator(codec, k, m)
    si = invert([g[v] for v in valid])
    rows = []
    for e in erased:
        rows.append([_dot(g[e], [si[j][i] for j in range(k)]) for i in range(k)])
    return rows


def _dot(a, b):
    r = 0
    for x, y in zip(a, b):
        r ^= mul(x, y)
    return r


def apply(rows, units):
    n = len(units[0])
    out = []
    for row in rows:
        tabs = [[mul(c, x) for x in range(256)] for c in row]
        o = bytearray(n)
        for tab, u in zip(tabs, units):
            for t in range(n):
                o[t] ^= tab[u[t]]
        out.append(bytes(o))
    return out


def pin_data(k: int, n: int):
    return [bytes((31 * j + 7 * t + 1) & 0xff for t in range(n)) for j in range(k)]


def check_pins():
    assert mul(0x53, 0xca) == 0x8f and mul(2, 0x80) == 0x1d and inv(2) == 0x8e and inv(3) == 0xf4
    rows = {
        (6, 3): ["7aba47a78ef4", "ba7aa747f48e", "ad9ddd983daa"],
        (3, 2): ["f48e01", "47a77a"],
        (10, 4): ["dd98ad9d5d963daa8ef4", "98dd9dad965daa3df48e", "3daa5d96ad9ddd9847a7", "aa3d965d9dad98dda747"],
    }
    for (k, m), want in rows.items():
        assert [bytes(r).hex() for r in parity_matrix("rs", k, m)] == want, (k, m)
    first = {
        (6, 3): ["127eb5a56ffa1909909005dcdf764c8c", "45836063ba0796601fc4d01a0a32e545",
                 "495c1c224a9e69132d8140f81611c834"],
        (3, 2): ["db285f394ed155334c148b0e9a1dc144", "9ae3a49c2dabeed6901682ef0bc0b1dc"],
        (10, 4): ["d65309429c5a9f8f5b0f83384843ae51"],
    }
    sha = {
        (6, 3): "d63542f1fd97d85fe9158c1909ef608d684100d7c5859687d09b5643050dd1c6",
        (3, 2): "4107e92190221677cecbfa7ac25fefac91467168674fa922809934f39138438a",
        (10, 4): "6966ad76a192941853707a506f2919bb392f62c2bb977987ed74c1af1a84676a",
    }
    for (k, m), want in first.items():
        par = apply(parity_matrix("rs", k, m), pin_data(k, 4096))
        for r, w in enumerate(want):
            assert par[r][:16].hex() == w, (k, m, r)
        assert hashlib.sha256(b"".join(par)).hexdigest() == sha[(k, m)], (k, m)


def main():
    check_pins()
    out = {"field": {"poly": 0x11d, "mul": [[0x53, 0xca, mul(0x53, 0xca)], [2, 0x80, mul(2, 0x80)], [0xff, 0xff, mul(0xff, 0xff)],
                                             [0x1d, 0x8e, mul(0x1d, 0x8e)]],
                     "inv": bytes(inv(a) for a in range(256)).hex()},
           "schemes": []}
    for codec, k, m in SCHEMES:
        par = apply(parity_matrix(codec, k, m), pin_data(k, 4096))
        # Every pattern of m erasures decoded from the first k survivors: the decode matrices
        # themselves.  All of them go into one digest (erased units, then the rows, pattern after
        # pattern in itertools.combinations order); the first, a middle and the last one are listed.
        digest = hashlib.sha256()
        every = list(itertools.combinations(range(k + m), m))
        patterns = []
        for i, erased in enumerate(every):
            valid = [u for u in range(k + m) if u not in erased][:k]
            rows = decode_matrix(codec, k, m, valid, erased)
            digest.update(bytes(erased) + b"".join(bytes(r) for r in rows))
            if i in (0, len(every) // 2, len(every) - 1):
                patterns.append({"erased": list(erased), "valid": valid, "rows": [bytes(r).hex() for r in rows]})
        out["schemes"].append({"codec": codec, "k": k, "m": m,
                               "parity_matrix": [bytes(r).hex() for r in parity_matrix(codec, k, m)],
                               "unit_bytes": 4096, "data": "unit j byte t = (31 j + 7 t + 1) & 0xff",
                               "parity_first16": [p[:16].hex() for p in par],
                               "parity_sha256": hashlib.sha256(b"".join(par)).hexdigest(),
                               "decode_patterns": len(every), "decode_sha256": digest.hexdigest(),
                               "decode": patterns})
    with open(os.path.join(HERE, "ec_rs.json"), "w") as f:
        # (one scheme per line)
        f.write('{"field": %s,\n "schemes": [\n  %s\n ]}\n' % (json.dumps(out["field"]),
                                                             ",\n  ".join(json.dumps(sc) for sc in out["schemes"])))


if __name__ == "__main__":
    main()
