#!/usr/bin/env python3
"""AES/CTR/NoPadding rates: the GPU calls (hdfs_aes_ctr_xor_strided_dev) beside
the derived LDS-lookup ceiling, the host path on one thread, and -- where the
box has it -- ``openssl speed``.

Each GPU row is captured into a HIP graph (`--inner` calls), the graph replayed
between two HIP events after a warm-up replay, `--windows` times (median, min,
max per call).  Every GPU output is compared with hdfs_aes_ctr_xor over the
same bytes on the host (whole buffers, guard bytes included); a mismatch makes
the tool fail.

The ceiling: the kernel makes 16 table lookups per round and 16-byte block
(160 / 192 / 224 for AES-128 / 192 / 256), ds_read_b32 serves 32 lanes per
clock and CU, so at most 32 * CUs * clock / lookups blocks per second:
about 2.0 / 1.6 / 1.4 TB/s on 256 CUs at 2.4 GHz.  Nothing here asserts a rate.

    python tools/aes_rate.py [--mib 256] [--out profiles/aes_rate.json]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOCK_HZ = 2.4e9
LOOKUPS_PER_CLK_CU = 32
GUARD = 0xEE


def ceiling_bytes_per_s(num_cu: int, rounds: int) -> float:
    return LOOKUPS_PER_CLK_CU * num_cu * CLOCK_HZ * 16 / (16 * rounds)


def replay_times(torch, calls, inner, outer, windows):
    """Per-replayed-sequence seconds of `calls(stream)` captured `inner` times: one per window."""
    s = torch.cuda.Stream()
    calls(s)  # (first launches outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(inner):
            calls(s)
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
    return sorted(out)


def stats(t, nbytes, ceiling=None):
    med = t[len(t) // 2]
    row = {"us": round(med * 1e6, 2), "us_min": round(t[0] * 1e6, 2), "us_max": round(t[-1] * 1e6, 2),
           "TBps": round(nbytes / med / 1e12, 4)}
    if ceiling:
        row["ceiling_TBps"] = round(ceiling / 1e12, 3)
        row["fraction_of_ceiling"] = round(nbytes / med / ceiling, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256, help="size of the large cases (config 2: 256)")
    ap.add_argument("--inner", type=int, default=5, help="calls captured into the graph")
    ap.add_argument("--outer", type=int, default=4, help="graph replays per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-mib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aes_rate.json"))
    args = ap.parse_args()
    import torch

    import oracle
    from bench import load_package

    hdfs = load_package()
    hdfs.lib()
    assert torch.cuda.is_available(), "aes_rate needs the GPU"
    ctx = hdfs.Context(0)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = args.mib << 20
    npk = n // 65536
    plain = oracle.xorshift64_bytes(n, oracle.SEED)
    src = torch.from_numpy(np.concatenate([plain, np.zeros(16, np.uint8)])).cuda()
    dst = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    iv = bytes(range(16))
    aes = {bits: hdfs.AesCtr(bytes(range(0x30, 0x30 + bits // 8)), iv) for bits in (128, 192, 256)}
    rows, bad = [], 0

    def gpu_row(name, bits, call, nbytes, segments):
        """segments: [(offset in dst, stream offset, source slice)] -- the expected image."""
        nonlocal bad
        dst.fill_(GUARD)
        t = replay_times(torch, call, args.inner, args.outer, args.windows)
        torch.cuda.synchronize()
        want = np.full(dst.numel(), GUARD, np.uint8)
        for off, so, a in segments:
            want[off:off + a.size] = aes[bits].xor(so, a)
        ok = bool(np.array_equal(dst.cpu().numpy(), want))
        bad += not ok
        row = {"case": name, "key_bits": bits, "bytes": nbytes, "matches_host": ok}
        row.update(stats(t, nbytes, ceiling_bytes_per_s(num_cu, aes[bits].rounds)))
        rows.append(row)
        return want

    so0 = 1 << 40
    for bits in (128, 192, 256):
        gpu_row("contiguous, phase 0", bits,
                lambda s, b=bits: ctx.aes_ctr_xor_strided(aes[b], src.data_ptr(), dst.data_ptr() + 16, n,
                                                          stream_off=so0, stream=s.cuda_stream),
                n, [(16, so0, plain)])
    gpu_row("contiguous, keystream phase 5, dst 5 bytes off", 128,
            lambda s: ctx.aes_ctr_xor_strided(aes[128], src.data_ptr(), dst.data_ptr() + 21, n, stream_off=so0 + 10,
                                              stream=s.cuda_stream),
            n, [(21, so0 + 10, plain)])
    stride = 65536 + 543
    gpu_row("wire shape: %d x 64 KiB, stream stride 65536 + 543" % npk, 128,
            lambda s: ctx.aes_ctr_xor_strided(aes[128], src.data_ptr(), dst.data_ptr() + 16, 65536, npk, 65536, 65536,
                                              so0 + 543, stride, stream=s.cuda_stream),
            n, [(16 + i * 65536, so0 + 543 + i * stride, plain[i * 65536:(i + 1) * 65536]) for i in range(npk)])
    blk = 4 << 20
    gpu_row("one 4 MiB block", 128,
            lambda s: ctx.aes_ctr_xor_strided(aes[128], src.data_ptr(), dst.data_ptr() + 16, blk, stream_off=so0,
                                              stream=s.cuda_stream),
            blk, [(16, so0, plain[:blk])])

    # the write step of an encryption zone: encrypt, then plan exec over the ciphertext
    pk = oracle.uniform_packets(npk, 65536, 512)
    nsums = hdfs.total_checksums(pk)
    sums = torch.zeros(nsums, dtype=torch.int32, device="cuda")
    plan = ctx.plan(pk)
    enc = lambda s: ctx.aes_ctr_xor_strided(aes[128], src.data_ptr(), dst.data_ptr() + 16, n, stream_off=so0,
                                            stream=s.cuda_stream)
    want = gpu_row("write step: encrypt, then plan exec over the ciphertext", 128,
                   lambda s: (enc(s), plan.exec(dst.data_ptr() + 16, sums.data_ptr(), s.cuda_stream)), n,
                   [(16, so0, plain)])
    got_sums = sums.cpu().numpy().view(np.uint32)
    sums_ok = bool(np.array_equal(got_sums, oracle.Oracle().batch(want[16:16 + n], pk, nsums)))
    bad += not sums_ok
    rows[-1]["checksums_match_oracle"] = sums_ok
    t = replay_times(torch, lambda s: plan.exec(dst.data_ptr() + 16, sums.data_ptr(), s.cuda_stream), args.inner,
                     args.outer, args.windows)
    row = {"case": "plan exec alone over the same ciphertext", "bytes": n}
    row.update(stats(t, n))
    rows.append(row)
    plan.close()

    # the host path, one thread
    hn = args.host_mib << 20
    hsrc, hout = plain[:hn], np.empty(hn, np.uint8)
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        aes[128].xor(so0, hsrc, hout)
        best = min(best, time.perf_counter() - t0)
    host = {"case": "hdfs_aes_ctr_xor, one host thread", "key_bits": 128, "bytes": hn, "ms": round(best * 1e3, 2),
            "GBps": round(hn / best / 1e9, 3)}

    ossl = None
    if shutil.which("openssl"):
        r = subprocess.run(["openssl", "speed", "-seconds", "1", "-bytes", "16384", "-evp", "aes-128-ctr"],
                           capture_output=True, text=True)
        last = [ln for ln in r.stdout.splitlines() if ln.lower().startswith("aes-128-ctr")]
        ossl = {"case": "openssl speed -evp aes-128-ctr (16384-byte blocks, one thread; the box's OpenSSL, AES-NI "
                        "where the CPU has it -- not this library)", "line": last[-1].strip() if last else r.stdout[-200:]}

    res = {"tool": "aes_rate", "device": torch.cuda.get_device_name(0), "num_cu": num_cu,
           "ceiling": "32 lookups/clk/CU * %d CUs * 2.4 GHz / (16 * rounds) blocks/s" % num_cu,
           "graph_launches": args.inner, "replays_per_window": args.outer, "windows": args.windows,
           "rows": rows, "host": host, "openssl": ossl, "mismatches": bad}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
