"""The pure logic of overlapping captured execs (csrc/capture_chain.h: the
range-overlap predicate, the independence rule, the run bookkeeping) built
with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/sanitize/capture_chain_host.cpp) and run: adjacent ranges, one byte of
overlap, empty ranges, ranges ending at the top of the address space, a
payload equal to the other exec's out, and the distinct-range cap forcing a
new run.  CPU only."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "native-hdfs-fuse_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_capture_chain_logic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "capture_chain_host")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "sanitize", "capture_chain_host.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "capture chain host run clean" in r.stdout
