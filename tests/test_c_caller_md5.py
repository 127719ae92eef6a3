"""The C caller of the block MD5-of-CRCs path (examples/file_checksum.c,
built by native-hdfs-fuse_amd/Makefile): a file's blocks in device memory,
crc32c_plan_exec_blocks_md5 per block shape, crc32c_file_md5 over the
digests.  The program checks every block digest against crc32c_block_md5
over crc32c() per chunk itself; here the file digest it prints is compared
with hashlib's over the oracle's checksums.  Run as a child process."""
from __future__ import annotations

import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "file_checksum")

# (nblocks, block_len, last_block_len, bpc): a file of 256 KiB blocks with a
# ragged last one; a single 4 MiB block; bpc 4096 with a last block shorter
# than one chunk.
CASES = [(5, 262144, 100000, 512), (1, 4194304, 4194304, 512), (3, 65536, 77, 4096)]


def expected_file_md5(orc, nblocks, block_len, last_len, bpc) -> str:
    """Block i holds the xorshift64 stream seeded with oracle.SEED + i (the fill
    examples/file_checksum.c states), cut into 64 KiB packets."""
    digests = []
    for i in range(nblocks):
        blen = last_len if i == nblocks - 1 else block_len
        data = oracle.xorshift64_bytes(blen, (oracle.SEED + i) & 0xFFFFFFFFFFFFFFFF)
        rows, pos, idx = [], 0, 0
        for plen in orc.packetize(blen, 0, 65536, bpc):
            if plen:
                rows.append((pos, idx, plen, bpc))
                pos += plen
                idx += -(-plen // bpc)
        wire = orc.batch(data, np.array(rows, dtype=oracle.PACKET_DTYPE), idx, big_endian=True)
        digests.append(hashlib.md5(wire.tobytes()).digest())
    return hashlib.md5(b"".join(digests)).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("nblocks,block_len,last_len,bpc", CASES)
def test_c_caller_file_checksum(orc, nblocks, block_len, last_len, bpc):
    if not os.path.exists(EXE):
        pytest.fail(EXE + " is not built (run __graft_entry__.build())")
    r = subprocess.run([EXE, str(nblocks), str(block_len), str(last_len), str(bpc)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
    assert r.stdout.split()[1] == expected_file_md5(orc, nblocks, block_len, last_len, bpc)
