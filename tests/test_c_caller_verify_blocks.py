"""The C caller of the multi-block verify path (examples/block_verify.c, built
by native-hdfs-fuse_amd/Makefile): blocks in device memory written with
crc32c_plan_exec_blocks, two of them corrupted, crc32c_plan_verify_blocks over
all of them.  The program checks every verdict and the bitmap itself; here
its report -- which blocks are bad and which bytes to fetch again -- is
compared with the corruption its header states.  Run as a child process."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "block_verify")

# (nblocks, block_len, bpc): the default 40 blocks (two launches); a ragged
# last chunk with bpc 4096.
CASES = [(40, 262144, 512), (35, 100000, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("nblocks,block_len,bpc", CASES)
def test_c_caller_block_verify(nblocks, block_len, bpc):
    if not os.path.exists(EXE):
        pytest.fail(EXE + " is not built (run __graft_entry__.build())")
    r = subprocess.run([EXE, str(nblocks), str(block_len), str(bpc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok: 2 of %d blocks bad" % nblocks, r.stdout
    n = -(-block_len // bpc)
    got = {}
    for line in lines[:-1]:
        m = re.fullmatch(r"bad block (\d+): (\d+) mismatches, re-fetch bytes \[(\d+), (\d+)\)", line)
        assert m, line
        got[int(m.group(1))] = tuple(int(x) for x in m.group(2, 3, 4))
    # block 7: chunks 3 and n - 2 (payload bytes); block 33: its last chunk (an expected word)
    assert got == {7: (2, 3 * bpc, (n - 1) * bpc), 33: (1, (n - 1) * bpc, block_len)}, r.stdout
