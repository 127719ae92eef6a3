"""The C caller of the composite-CRC path (examples/file_composite_crc.c,
built by native-hdfs-fuse_amd/Makefile): a file's blocks in device memory,
crc32c_plan_exec_blocks_composite per block shape, crc32c_file_composite over
the block CRCs.  The program checks every block CRC and the file CRC against
the scalar crc32c() over the bytes itself; here the value it prints is
compared with the oracle's CRC of the same file.  Run as a child process."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "file_composite_crc")

# (nblocks, block_len, last_block_len, bpc): a file of 256 KiB blocks with a
# ragged last one; a single 4 MiB block; bpc 4096 with a last block shorter
# than one chunk.
CASES = [(5, 262144, 100000, 512), (1, 4194304, 4194304, 512), (3, 65536, 77, 4096)]


def expected_file_crc(orc, nblocks, block_len, last_len) -> int:
    """Block i holds the xorshift64 stream seeded with oracle.SEED + i (the fill
    examples/file_composite_crc.c states)."""
    blocks = [oracle.xorshift64_bytes(last_len if i == nblocks - 1 else block_len,
                                      (oracle.SEED + i) & 0xFFFFFFFFFFFFFFFF) for i in range(nblocks)]
    return orc.crc32c(np.concatenate(blocks))


@pytest.mark.gpu
@pytest.mark.parametrize("nblocks,block_len,last_len,bpc", CASES)
def test_c_caller_file_composite_crc(orc, nblocks, block_len, last_len, bpc):
    if not os.path.exists(EXE):
        pytest.fail(EXE + " is not built (run __graft_entry__.build())")
    r = subprocess.run([EXE, str(nblocks), str(block_len), str(last_len), str(bpc)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
    assert int(r.stdout.split()[1], 16) == expected_file_crc(orc, nblocks, block_len, last_len)
