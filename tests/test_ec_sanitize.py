"""The host erasure-coding sources (csrc/ec_gf256.h, csrc/ec_host.cpp) built
with AddressSanitizer + UndefinedBehaviorSanitizer together with the
stand-alone program tests/sanitize/ec_host.cpp (its own main: known answers,
every RS(6,3) erasure pattern, unaligned pointers, NULL inputs, buffers that
end where their allocation ends).  CPU only; the program is run directly."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "native-hdfs-fuse_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_ec_host_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ec_host")
    srcs = [os.path.join(CSRC, f) for f in ("errors.cpp", "ec_host.cpp")]
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "sanitize", "ec_host.cpp"), *srcs, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ec host sanitizer run clean" in r.stdout
