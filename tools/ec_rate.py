#!/usr/bin/env python3
"""Erasure-coding rates: the GPU calls (hdfs_ec_encode_striped_dev,
hdfs_ec_apply_dev) beside the two derived ceilings and a plain device copy of
the same traffic in the same run, the host path on one thread, and the unit
length from which one GPU call beats the host loop.

Each GPU row is captured into a HIP graph (`--inner` calls), the graph replayed
between two HIP events after a warm-up replay, `--windows` times (median, min,
max per call).  Every GPU output is compared with hdfs_ec_apply over the same
bytes on the host (whole buffers, guard bytes included); a mismatch makes the
tool fail.  Nothing here asserts a rate.

The ceilings (derived, not measured).  HBM: an encode reads the data once and
writes m / k of it, (k + m) / k bytes of traffic per data byte, against the
8.0 TB/s of the datasheet.  LDS: two nibble lookups per data byte, ds_read_b32
serves 32 lanes per clock and CU: 16 data bytes per clock and CU, 9.8 TB/s on
256 CUs at 2.4 GHz.  The yardstick is what a plain device-to-device copy
reaches in the same run: a copy of traffic / 2 bytes moves the same bytes.

    python tools/ec_rate.py [--mib 192] [--out profiles/ec_rate.json]
    python tools/ec_rate.py --pmc-workload     # plain launches for a counter run of its own

The counter run and its summary (profiles/ec_pmc.json):

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d OUT -o ec --output-format csv -- \
        python tools/ec_rate.py --pmc-workload
    python tools/ec_rate.py --pmc-summary OUT [--out profiles/ec_pmc.json]     # no GPU needed
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOCK_HZ = 2.4e9
HBM_PEAK = 8.0e12
LOOKUPS_PER_CLK_CU = 32
GUARD = 0xEE
CELL = 1 << 20
SCHEMES = [(6, 3), (10, 4), (3, 2)]


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


def stats(t, data_bytes, traffic):
    med = t[len(t) // 2]
    return {"us": round(med * 1e6, 2), "us_min": round(t[0] * 1e6, 2), "us_max": round(t[-1] * 1e6, 2),
            "data_TBps": round(data_bytes / med / 1e12, 4), "traffic_TBps": round(traffic / med / 1e12, 4)}


def host_striped_parity(hdfs, mx, buf, cell):
    k = mx.n_in
    plen = hdfs.ec_group_layout(buf.size, k, mx.n_out, cell)[k]
    par = [np.zeros(plen, np.uint8) for _ in range(mx.n_out)]
    for s in range(-(-buf.size // (k * cell))):
        n = min(cell, buf.size - s * k * cell)
        cells = []
        for j in range(k):
            c = buf[(s * k + j) * cell:(s * k + j + 1) * cell][:n]
            cells.append(None if c.size == 0 else np.concatenate([c, np.zeros(n - c.size, np.uint8)]))
        for r, o in enumerate(mx.apply(cells)):
            par[r][s * cell:s * cell + n] = o
    return par


def pmc_workload(torch, hdfs, ctx, oracle):
    """Three launches of the striped RS-6-3 encode over 48 MiB, everything aligned, and three of a
    3-erasure decode with every pointer at its own phase; outputs compared with the host's."""
    k, m = 6, 3
    enc = hdfs.EcMatrix.encode(k, m)
    n = 48 << 20
    buf = oracle.xorshift64_bytes(n, oracle.SEED)
    src = torch.from_numpy(np.concatenate([buf, np.zeros(32, np.uint8)])).cuda()
    plen = n // k
    par = torch.full((m * (plen + 64),), GUARD, dtype=torch.uint8, device="cuda")
    outs = [par.data_ptr() + 16 + r * (plen + 64) for r in range(m)]
    for _ in range(3):
        ctx.ec_encode_striped(enc, src.data_ptr(), n, CELL, outs)
    torch.cuda.synchronize()
    want = host_striped_parity(hdfs, enc, buf, CELL)
    h = par.cpu().numpy()
    ok = all(np.array_equal(h[16 + r * (plen + 64):16 + r * (plen + 64) + plen], want[r]) for r in range(m))
    dec = hdfs.EcMatrix.decode(k, m, [0, 2, 3, 5, 6, 8], [1, 4, 7])
    u = 4 << 20
    ins = [src.data_ptr() + j * (u + 16) + j + 1 for j in range(k)]
    douts = [par.data_ptr() + 32 + r * (plen + 64) + 5 * r + 3 for r in range(m)]
    for _ in range(3):
        ctx.ec_apply(dec, ins, douts, u)
    torch.cuda.synchronize()
    wd = dec.apply([buf[j * (u + 16) + j + 1:j * (u + 16) + j + 1 + u] for j in range(k)])
    h = par.cpu().numpy()
    for r in range(m):
        o = 32 + r * (plen + 64) + 5 * r + 3
        ok = ok and bool(np.array_equal(h[o:o + u], wd[r]))
    print(json.dumps({"pmc_workload": "3 x striped RS-6-3 encode of 48 MiB (aligned), 3 x 3-erasure decode of 4 MiB "
                                      "units (every pointer at its own phase)", "matches_host": bool(ok)}))
    return 0 if ok else 1


PMC_COMMAND = ("rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d OUT -o ec --output-format csv -- "
               "python tools/ec_rate.py --pmc-workload (a run of its own); python tools/ec_rate.py --pmc-summary OUT")


def pmc_summary(directory, out):
    """The *counter_collection.csv files under `directory` (rocprofv3's output of the --pmc-workload
    run) as one JSON line: per counter the values of the striped and of the apply launches in order."""
    import csv
    import glob

    files = sorted(glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True))
    if not files:
        print("no *counter_collection.csv under " + directory, file=sys.stderr)
        return 1
    launches = {}  # dispatch id -> (form, {counter: value})
    for path in files:
        with open(path) as f:
            for row in csv.DictReader(f):
                if "hdfs_ec_kernel" not in row["Kernel_Name"]:
                    continue
                form = "striped" if "<true>" in row["Kernel_Name"] else "apply"
                launches.setdefault(int(row["Dispatch_Id"]), (form, {}))[1][row["Counter_Name"]] = int(float(row["Counter_Value"]))
    res = {"tool": PMC_COMMAND,
           "workload": "3 launches of hdfs_ec_encode_striped_dev, RS-6-3, 48 MiB of data in 1 MiB cells, everything "
                       "aligned; 3 launches of hdfs_ec_apply_dev, a 3-erasure RS-6-3 decode of 4 MiB units with every "
                       "pointer at its own phase; outputs equal to the host's",
           "kernels": {"striped": "hdfs_ec_kernel<true>", "apply": "hdfs_ec_kernel<false>"}}
    for name in ("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"):
        res[name] = {form: [c[name] for _, (f, c) in sorted(launches.items()) if f == form and name in c]
                     for form in ("striped", "apply")}
    line = json.dumps(res)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=192, help="data bytes of the large cases")
    ap.add_argument("--inner", type=int, default=5, help="calls captured into the graph")
    ap.add_argument("--outer", type=int, default=4, help="graph replays per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-mib", type=int, default=12)
    ap.add_argument("--pmc-workload", action="store_true")
    ap.add_argument("--pmc-summary", metavar="DIR", help="summarise rocprofv3's counter CSVs under DIR (no GPU)")
    ap.add_argument("--out", default=None, help="default: profiles/ec_rate.json (--pmc-summary: profiles/ec_pmc.json)")
    args = ap.parse_args()
    if args.pmc_summary:
        return pmc_summary(args.pmc_summary, args.out or os.path.join(ROOT, "profiles", "ec_pmc.json"))
    args.out = args.out or os.path.join(ROOT, "profiles", "ec_rate.json")
    import torch

    import oracle
    from bench import load_package

    hdfs = load_package()
    hdfs.lib()
    assert torch.cuda.is_available(), "ec_rate needs the GPU"
    ctx = hdfs.Context(0)
    if args.pmc_workload:
        return pmc_workload(torch, hdfs, ctx, oracle)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lds_ceiling = LOOKUPS_PER_CLK_CU / 2 * num_cu * CLOCK_HZ  # data bytes / s
    n = args.mib << 20
    data = oracle.xorshift64_bytes(n, oracle.SEED)
    src = torch.from_numpy(np.concatenate([data, np.zeros(32, np.uint8)])).cuda()
    pitch = n + 4 * CELL
    dst = torch.full((pitch,), GUARD, dtype=torch.uint8, device="cuda")
    copy_src = torch.empty(n, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    rows, bad = [], 0

    def copy_row(traffic):
        """A device-to-device copy that moves `traffic` bytes (reads half, writes half)."""
        half = min(int(traffic // 2), n)
        a, b = copy_src[:half], copy_dst[:half]

        def call(s):
            with torch.cuda.stream(s):
                b.copy_(a)

        t = replay_times(torch, call, args.inner, args.outer, args.windows)
        med = t[len(t) // 2]
        return {"copy_bytes": half, "copy_us": round(med * 1e6, 2), "copy_traffic_TBps": round(2 * half / med / 1e12, 4)}

    def gpu_row(name, call, data_bytes, traffic, k, m, expected):
        """expected: [(offset in dst, bytes)] -- the expected image."""
        nonlocal bad
        dst.fill_(GUARD)
        t = replay_times(torch, call, args.inner, args.outer, args.windows)
        torch.cuda.synchronize()
        want = np.full(dst.numel(), GUARD, np.uint8)
        for off, a in expected:
            want[off:off + a.size] = a
        ok = bool(np.array_equal(dst.cpu().numpy(), want))
        bad += not ok
        row = {"case": name, "k": k, "m": m, "data_bytes": data_bytes, "traffic_bytes": traffic, "matches_host": ok}
        row.update(stats(t, data_bytes, traffic))
        row["hbm_ceiling_data_TBps"] = round(HBM_PEAK * data_bytes / traffic / 1e12, 3)
        row["lds_ceiling_data_TBps"] = round(lds_ceiling / 1e12, 3)
        row.update(copy_row(traffic))
        row["time_over_copy"] = round(row["us"] / row["copy_us"], 3)
        rows.append(row)
        return row

    def striped_case(name, k, m, length):
        mx = hdfs.EcMatrix.encode(k, m)
        par = host_striped_parity(hdfs, mx, data[:length], CELL)
        plen = par[0].size
        slot = (plen + 4096 + 15) // 16 * 16
        outs = [dst.data_ptr() + 16 + r * slot for r in range(m)]
        return gpu_row(name, lambda s: ctx.ec_encode_striped(mx, src.data_ptr(), length, CELL, outs, stream=s.cuda_stream),
                       length, length + m * plen, k, m, [(16 + r * slot, par[r]) for r in range(m)])

    for k, m in SCHEMES:
        striped_case("encode RS-%d-%d, %d MiB of data, 1 MiB cells" % (k, m, args.mib), k, m, n)
    striped_case("encode RS-6-3, one 6 MiB stripe", 6, 3, 6 * CELL)

    # a 3-erasure decode of RS-6-3: six surviving internal blocks, three rebuilt
    k, m = 6, 3
    u = n // k
    dec = hdfs.EcMatrix.decode(k, m, [0, 2, 3, 5, 6, 8], [1, 4, 7])
    ins = [src.data_ptr() + j * u for j in range(k)]
    slot = u + 4096
    wd = dec.apply([data[j * u:(j + 1) * u] for j in range(k)])
    gpu_row("decode RS-6-3, 3 erasures, units of %d MiB" % (u >> 20),
            lambda s: ctx.ec_apply(dec, ins, [dst.data_ptr() + 16 + r * slot for r in range(m)], u, stream=s.cuda_stream),
            k * u, (k + m) * u, k, m, [(16 + r * slot, wd[r]) for r in range(m)])

    # the write step: encode, then the nine internal blocks' checksums
    enc = hdfs.EcMatrix.encode(k, m)
    par = host_striped_parity(hdfs, enc, data, CELL)
    plen = par[0].size
    slot = (plen + 4096 + 15) // 16 * 16
    pouts = [dst.data_ptr() + 16 + r * slot for r in range(m)]
    pkts = [hdfs.ec_block_packets(n, k, CELL, b, 65536, 512) for b in range(k)]
    ppk = oracle.uniform_packets(plen // 65536, 65536, 512)
    plans = [ctx.plan(pk) for pk in pkts] + [ctx.plan(ppk)]
    nsums = plen // 512
    sums = torch.zeros((k + m, nsums), dtype=torch.int32, device="cuda")

    def checksums(s):
        for b in range(k):
            plans[b].exec(src.data_ptr(), sums[b].data_ptr(), s.cuda_stream)
        for r in range(m):
            plans[k].exec(pouts[r], sums[k + r].data_ptr(), s.cuda_stream)

    def write_step(s):
        ctx.ec_encode_striped(enc, src.data_ptr(), n, CELL, pouts, stream=s.cuda_stream)
        checksums(s)

    row = gpu_row("write step RS-6-3: encode, then the nine internal blocks' plan exec", write_step, n, n + m * plen, k, m,
                  [(16 + r * slot, par[r]) for r in range(m)])
    orc = oracle.Oracle()
    got = sums.cpu().numpy().view(np.uint32)
    ncell = n // CELL
    blocks = [np.concatenate([data[i * CELL:(i + 1) * CELL] for i in range(b, ncell, k)]) for b in range(k)] + par
    sums_ok = all(np.array_equal(got[i], orc.chunks(np.ascontiguousarray(blocks[i]), 512)) for i in range(k + m))
    bad += not sums_ok
    row["checksums_match_oracle"] = bool(sums_ok)
    t = replay_times(torch, checksums, args.inner, args.outer, args.windows)
    r2 = {"case": "the nine plan execs alone", "data_bytes": n}
    r2.update(stats(t, n, n + m * plen))
    rows.append(r2)
    for p in plans:
        p.close()

    # the host path, one thread, and the unit length from which one GPU call beats it
    hn = (args.host_mib << 20) // k
    hin = [data[j * hn:(j + 1) * hn] for j in range(k)]
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        enc.apply(hin)
        best = min(best, time.perf_counter() - t0)
    host = {"case": "hdfs_ec_apply RS-6-3, one host thread", "data_bytes": k * hn, "ms": round(best * 1e3, 2),
            "data_GBps": round(k * hn / best / 1e9, 3)}
    cross = []
    outs_h = [np.empty(1 << 20, np.uint8) for _ in range(m)]
    for lg in range(6, 17):
        ln = 1 << lg
        reps = 20
        ptr_in = [data[j * (1 << 20):].ctypes.data for j in range(k)]
        ptr_out = [o.ctypes.data for o in outs_h]
        t0 = time.perf_counter()
        for _ in range(reps):
            enc.apply_ptrs(ptr_in, ptr_out, ln)
        th = (time.perf_counter() - t0) / reps
        gouts = [dst.data_ptr() + 16 + r * slot for r in range(m)]
        gins = [src.data_ptr() + j * (1 << 20) for j in range(k)]
        ctx.ec_apply(enc, gins, gouts, ln)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.ec_apply(enc, gins, gouts, ln)
            torch.cuda.synchronize()
        tg = (time.perf_counter() - t0) / reps
        cross.append({"unit_bytes": ln, "host_us": round(th * 1e6, 2), "gpu_call_and_sync_us": round(tg * 1e6, 2)})
    first = next((c["unit_bytes"] for c in cross if c["gpu_call_and_sync_us"] < c["host_us"]), None)

    res = {"tool": "ec_rate", "device": torch.cuda.get_device_name(0), "num_cu": num_cu,
           "ceilings": "HBM: 8.0 TB/s * k / (k + m) data bytes/s; LDS: 32 lookups/clk/CU / 2 per byte * %d CUs * 2.4 GHz" % num_cu,
           "graph_launches": args.inner, "replays_per_window": args.outer, "windows": args.windows,
           "rows": rows, "host": host, "gpu_vs_host_loop": cross, "gpu_call_beats_host_from_unit_bytes": first,
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
