#!/usr/bin/env python3
"""Composite CRCs: the GPU call (crc32c_composite_cells) against the host loop
(crc32c_block_composite on one thread) over the same checksum arrays.

For each case (cells x checksums per cell, bpc 512): random checksums in
device memory; composite_cells captured into a HIP graph (`--inner` calls),
the graph replayed between two HIP events after a warm-up replay, `--windows`
times (median, min, max per call); then crc32c_block_composite per cell on one
host thread over the same arrays (best of the repetitions).  Every result of
every run (GPU and host) is compared: the GPU's outputs after the last replay
with the host values, and the host values of every repetition with the first.
Prints one JSON line (and writes it to --out).

    python tools/composite_rate.py [--cases 1x8192,1x262144,...] [--out profiles/composite_rate.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BPC = 512
CASES = "1x8192,1x262144,64x8192,1024x8192,8192x8192,4096x128"


def gpu_times(torch, ctx, dsums, nsums, cpc, dcrcs, inner, outer, windows):
    """Per-call seconds of composite_cells, graph-replayed: one per window."""
    s = torch.cuda.Stream()
    call = lambda: ctx.composite_cells(dsums.data_ptr(), nsums, cpc, BPC, BPC, dcrcs.data_ptr(), 0, s.cuda_stream)
    call()  # (first launch outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(inner):
            call()
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


def host_loop(hdfs, sums, ncells, cpc, reps):
    """Best wall seconds of crc32c_block_composite over every cell, one thread; the values; whether
    every repetition gave the same."""
    f = hdfs.lib().crc32c_block_composite
    crcs = np.zeros(ncells, np.uint32)
    src, dst = sums.ctypes.data, crcs.ctypes.data
    calls = [(ctypes.c_void_p(src + 4 * cpc * i), ctypes.c_void_p(dst + 4 * i)) for i in range(ncells)]
    best, first, same = float("inf"), None, True
    for _ in range(reps):
        crcs[:] = 0
        t0 = time.perf_counter()
        for a, d in calls:
            f(a, cpc, BPC, BPC, 0, d)
        best = min(best, time.perf_counter() - t0)
        if first is None:
            first = crcs.copy()
        same = same and np.array_equal(first, crcs)
    return best, first, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES, help="cells x checksums per cell, comma separated")
    ap.add_argument("--inner", type=int, default=10, help="calls captured into the graph")
    ap.add_argument("--outer", type=int, default=5, help="graph replays per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_rate.json"))
    args = ap.parse_args()
    import torch

    from bench import load_package

    hdfs = load_package()
    hdfs.lib()
    assert torch.cuda.is_available(), "composite_rate needs the GPU"
    ctx = hdfs.Context(0)
    rng = np.random.default_rng(8192)
    rows, bad = [], 0
    for case in args.cases.split(","):
        ncells, cpc = (int(x) for x in case.split("x"))
        sums = rng.integers(0, 1 << 32, ncells * cpc, dtype=np.uint64).astype(np.uint32)
        dsums = torch.from_numpy(sums.view(np.int32)).cuda()
        dcrcs = torch.zeros(ncells, dtype=torch.int32, device="cuda")
        reps = max(3, min(50, int(0.3 / (2.5e-9 * sums.size + 1e-6 * ncells))))
        host_s, want, host_ok = host_loop(hdfs, sums, ncells, cpc, reps)
        t = sorted(gpu_times(torch, ctx, dsums, sums.size, cpc, dcrcs, args.inner, args.outer, args.windows))
        gpu_ok = bool(np.array_equal(dcrcs.cpu().numpy().view(np.uint32), want))
        bad += (not gpu_ok) + (not host_ok)
        med = t[len(t) // 2]
        rows.append({"cells": ncells, "crc_per_cell": cpc, "gpu_us": round(med * 1e6, 2),
                     "gpu_us_min": round(t[0] * 1e6, 2), "gpu_us_max": round(t[-1] * 1e6, 2),
                     "gpu_ns_per_checksum": round(med * 1e9 / sums.size, 4),
                     "host_us": round(host_s * 1e6, 2), "host_ns_per_checksum": round(host_s * 1e9 / sums.size, 4),
                     "gpu_matches_host": gpu_ok, "host_repeatable": host_ok})
        del dsums, dcrcs
    res = {"tool": "composite_rate", "bpc": BPC, "device": torch.cuda.get_device_name(0),
           "graph_launches": args.inner, "replays_per_window": args.outer, "windows": args.windows,
           "rows": rows, "cases_gpu_faster": [[r["cells"], r["crc_per_cell"]] for r in rows if r["gpu_us"] < r["host_us"]],
           "mismatches": bad}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
