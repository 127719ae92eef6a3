#!/usr/bin/env python3
"""Block MD5-of-CRCs: the GPU call (crc32c_md5_blocks) against the host loop
(crc32c_block_md5 on one thread) over the same checksum arrays.

For crc_per_block = 8192 (a 4 MiB block of 512-byte chunks) and each block
count: random checksums in device memory; md5_blocks captured into a HIP
graph (`--inner` launches), the graph replayed between two HIP events after a
warm-up replay, `--windows` times (median, min, max per call); then
crc32c_block_md5 per block on one host thread over the same arrays (best of
the repetitions).  Every digest of every run (GPU and host) is checked
against hashlib.  Prints one JSON line (and writes it to --out).

    python tools/md5_rate.py [--blocks 1,32,64,1024,8192] [--out profiles/md5_rate.json]
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CPB = 8192


def gpu_times(torch, ctx, dsums, nsums, dmd5, inner, outer, windows):
    """Per-call seconds of md5_blocks, graph-replayed: one per window."""
    s = torch.cuda.Stream()
    ctx.md5_blocks(dsums.data_ptr(), nsums, CPB, dmd5.data_ptr(), 0, s.cuda_stream)  # (first launch outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(inner):
            ctx.md5_blocks(dsums.data_ptr(), nsums, CPB, dmd5.data_ptr(), 0, s.cuda_stream)
    out = []
    with torch.cuda.stream(s):
        g.replay()  # warm-up
        s.synchronize()
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(outer):
                g.replay()
            e1.record(s)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3 / (inner * outer))
    del g
    return out


def host_loop(hdfs, sums, nblocks, reps):
    """Best wall seconds of crc32c_block_md5 over every block, one thread; the digests."""
    f = hdfs.lib().crc32c_block_md5
    md5 = np.zeros(16 * nblocks, np.uint8)
    src, dst = sums.ctypes.data, md5.ctypes.data
    calls = [(ctypes.c_void_p(src + 4 * CPB * i), ctypes.c_void_p(dst + 16 * i)) for i in range(nblocks)]
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for a, d in calls:
            f(a, CPB, 0, d)
        best = min(best, time.perf_counter() - t0)
    return best, md5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="1,2,4,8,16,32,64,1024,8192")
    ap.add_argument("--inner", type=int, default=10, help="launches captured into the graph")
    ap.add_argument("--outer", type=int, default=5, help="graph replays per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md5_rate.json"))
    args = ap.parse_args()
    import torch

    from bench import load_package

    hdfs = load_package()
    hdfs.lib()
    assert torch.cuda.is_available(), "md5_rate needs the GPU"
    ctx = hdfs.Context(0)
    rng = np.random.default_rng(8192)
    rows, bad = [], 0
    for nb in [int(x) for x in args.blocks.split(",")]:
        sums = rng.integers(0, 1 << 32, nb * CPB, dtype=np.uint64).astype(np.uint32)
        be = sums.astype(">u4")
        want = b"".join(hashlib.md5(be[i * CPB:(i + 1) * CPB].tobytes()).digest() for i in range(nb))
        dsums = torch.from_numpy(sums.view(np.int32)).cuda()
        dmd5 = torch.zeros(16 * nb, dtype=torch.uint8, device="cuda")
        t = sorted(gpu_times(torch, ctx, dsums, sums.size, dmd5, args.inner, args.outer, args.windows))
        gpu_ok = dmd5.cpu().numpy().tobytes() == want
        reps = max(3, min(200, int(0.3 / (45e-6 * nb))))
        host_s, host_md5 = host_loop(hdfs, sums, nb, reps)
        host_ok = host_md5.tobytes() == want
        bad += (not gpu_ok) + (not host_ok)
        rows.append({"blocks": nb, "gpu_us": round(t[len(t) // 2] * 1e6, 2), "gpu_us_min": round(t[0] * 1e6, 2),
                     "gpu_us_max": round(t[-1] * 1e6, 2), "gpu_us_per_block": round(t[len(t) // 2] * 1e6 / nb, 3),
                     "host_us": round(host_s * 1e6, 2), "host_us_per_block": round(host_s * 1e6 / nb, 3),
                     "gpu_digests_ok": gpu_ok, "host_digests_ok": host_ok})
        del dsums, dmd5
    faster = [r["blocks"] for r in rows if r["gpu_us"] < r["host_us"]]
    res = {"tool": "md5_rate", "crc_per_block": CPB, "device": torch.cuda.get_device_name(0),
           "graph_launches": args.inner, "replays_per_window": args.outer, "windows": args.windows,
           "rows": rows, "smallest_measured_count_gpu_faster": min(faster) if faster else None,
           "digest_mismatches": bad}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
