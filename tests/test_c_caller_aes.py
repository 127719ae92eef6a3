"""The C caller of the AES/CTR path (examples/encrypted_block.c, built by
native-hdfs-fuse_amd/Makefile): a block of an encryption-zone file in device
memory -- encrypt, checksum the ciphertext with a plan, combine, verify,
decrypt in place.  The program checks the ciphertext against the host path,
the round trip against the plaintext and the composite CRC against the scalar
crc32c() itself; here the value it prints is compared with the oracle's CRC of
the host-encrypted block.  Run as a child process."""
from __future__ import annotations

import os
import subprocess

import pytest

import oracle
from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "encrypted_block")

# (block_len, bpc, file_offset, key_bits): a 1 MiB block at a block boundary of the file; a ragged
# block at an odd file offset under each of the other key sizes.
CASES = [(1 << 20, 512, 128 << 20, 128), (300000, 4096, (1 << 40) + 5, 192), (65536 + 77, 512, 3, 256)]


def expected_crc(hdfs, orc, block_len, file_off, key_bits) -> int:
    """The fill, key and IV examples/encrypted_block.c states."""
    plain = oracle.xorshift64_bytes(block_len, oracle.SEED)
    aes = hdfs.AesCtr(bytes(range(key_bits // 8)), bytes(range(0xf0, 0x100)))
    return orc.crc32c(aes.xor(file_off, plain))


@pytest.mark.gpu
@pytest.mark.parametrize("block_len,bpc,file_off,key_bits", CASES)
def test_c_caller_encrypted_block(hdfs, orc, block_len, bpc, file_off, key_bits):
    if not os.path.exists(EXE):
        pytest.fail(EXE + " is not built (run __graft_entry__.build())")
    r = subprocess.run([EXE, str(block_len), str(bpc), str(file_off), str(key_bits)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
    assert int(r.stdout.split()[1], 16) == expected_crc(hdfs, orc, block_len, file_off, key_bits)
