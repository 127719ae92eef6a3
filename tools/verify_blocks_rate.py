#!/usr/bin/env python3
"""Verifying many blocks: one crc32c_plan_verify_blocks call against a loop of
crc32c_plan_verify_bitmap calls, one per block, over the same blocks.

The config-3 block shape (4 MiB, 64 KiB packets, bpc 512: 8192 checksums) at
1, 8, 32, 256 and 1024 blocks with distinct payloads (random bytes made on the
device).  The expected checksums are what crc32c_plan_exec_blocks wrote for
the same blocks.  Three things are timed in one run, their windows
alternating, host-issued and graph-replayed, with HIP events:
  (a) per_block: crc32c_plan_verify_bitmap once per block -- the baseline:
      existing code, one result pair and one bitmap per block;
  (b) verify_blocks: crc32c_plan_verify_blocks -- one verify launch per 32
      blocks and one verdict launch;
  (c) exec_blocks: crc32c_plan_exec_blocks, for scale.
Host-issued calls go through ctypes with their arguments built beforehand (a
C caller pays less per call); a graph replay has no per-call host cost.  The
timed windows start after `--warmup` calls of each kind (steady state, not
the first launches).  Every configuration is also checked once: clean data
gives clean verdicts / results, and one flipped payload byte gives exactly
that block and chunk, from (a) and from (b).
Prints one JSON line (and writes it to --out).

    python tools/verify_blocks_rate.py [--blocks 1,8,32,256,1024] [--out profiles/verify_blocks_rate.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK_BYTES, PACKET, BPC = 4 << 20, 65536, 512
NONE = 0xFFFFFFFF


def timed(torch, s, fn, reps):
    """Seconds per call of fn, `reps` calls between two events on stream s."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record(s)
        for _ in range(reps):
            fn()
        e1.record(s)
        e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def captured(torch, s, fn):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    return g


def stats(ts, nblocks):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"us": round(med * 1e6, 2), "us_min": round(ts[0] * 1e6, 2), "us_max": round(ts[-1] * 1e6, 2),
            "us_per_block": round(med * 1e6 / nblocks, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="1,8,32,256,1024")
    ap.add_argument("--warmup", type=int, default=60, help="calls of each kind before its first timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=512, help="per-block launches a timed window should hold at least")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_blocks_rate.json"))
    args = ap.parse_args()
    import torch

    from bench import load_package

    hdfs = load_package()
    L = hdfs.lib()
    assert torch.cuda.is_available(), "verify_blocks_rate needs the GPU"
    counts = [int(x) for x in args.blocks.split(",")]
    nmax = max(counts)
    ctx = hdfs.Context(0)
    rows_pk = [(PACKET * i, (PACKET // BPC) * i, PACKET, BPC) for i in range(BLOCK_BYTES // PACKET)]
    pk = np.array(rows_pk, dtype=hdfs.PACKET_DTYPE)
    plan = ctx.plan(pk, 0)
    n = plan.nchecksums
    bm_words = -(-n // 32)
    vp = ctypes.c_void_p

    # distinct payloads, one allocation; the expected checksums from exec_blocks
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4096)
    pay = torch.randint(0, 256, (nmax * BLOCK_BYTES + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    ptrs = [pay.data_ptr() + BLOCK_BYTES * b for b in range(nmax)]
    expected = torch.zeros(nmax * n, dtype=torch.int32, device="cuda")
    outs = [expected.data_ptr() + 4 * n * b for b in range(nmax)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.exec_blocks(ptrs, outs, s.cuda_stream)
    s.synchronize()
    scratch = torch.zeros(nmax * n, dtype=torch.int32, device="cuda")  # exec_blocks' timed output
    souts = [scratch.data_ptr() + 4 * n * b for b in range(nmax)]

    rows, bad = [], 0
    for nb in counts:
        verdicts = torch.full((nb * 4,), -1, dtype=torch.int32, device="cuda")
        work = torch.full((plan.verify_blocks_work_bytes(nb) // 4,), -1, dtype=torch.int32, device="cuda")
        res = torch.full((nb * 2,), -1, dtype=torch.int32, device="cuda")
        bms = torch.full((nb * bm_words,), -1, dtype=torch.int32, device="cuda")
        sh = vp(s.cuda_stream)
        per_args = [(plan.handle, vp(ptrs[b]), vp(outs[b]), vp(res.data_ptr() + 8 * b),
                     vp(bms.data_ptr() + 4 * bm_words * b), sh) for b in range(nb)]
        pays = (vp * nb)(*[vp(p) for p in ptrs[:nb]])
        out_arr = (vp * nb)(*[vp(p) for p in souts[:nb]])
        f_per, f_blocks, f_exec = L.crc32c_plan_verify_bitmap, L.crc32c_plan_verify_blocks, L.crc32c_plan_exec_blocks

        def per_block():
            for a in per_args:
                if f_per(*a):
                    raise RuntimeError(L.crc32c_last_error())

        def verify_blocks():
            if f_blocks(plan.handle, pays, vp(expected.data_ptr()), nb, vp(verdicts.data_ptr()), vp(work.data_ptr()), sh):
                raise RuntimeError(L.crc32c_last_error())

        def exec_blocks():
            if f_exec(plan.handle, pays, out_arr, nb, sh):
                raise RuntimeError(L.crc32c_last_error())

        # correctness, once per configuration: clean, then one corrupted block
        def outcome():
            per_block()
            verify_blocks()
            s.synchronize()
            v = verdicts.cpu().numpy().view(np.uint32).reshape(nb, 4)
            r = res.cpu().numpy().view(np.uint32).reshape(nb, 2)
            return v, r

        torch.cuda.synchronize()
        v, r = outcome()
        clean_ok = bool((v == np.array([0, NONE, NONE, 0], np.uint32)).all() and (r == np.array([0, NONE], np.uint32)).all())
        hit, chunk = nb // 2, 5
        at = hit * BLOCK_BYTES + chunk * BPC + 3
        pay[at] = pay[at] ^ 0x10
        torch.cuda.synchronize()
        v, r = outcome()
        want_v = np.tile(np.array([0, NONE, NONE, 0], np.uint32), (nb, 1))
        want_v[hit] = (1, chunk, chunk, 0)
        want_r = np.tile(np.array([0, NONE], np.uint32), (nb, 1))
        want_r[hit] = (1, chunk)
        corrupt_ok = bool((v == want_v).all() and (r == want_r).all())
        pay[at] = pay[at] ^ 0x10
        torch.cuda.synchronize()
        bad += (not clean_ok) + (not corrupt_ok)

        kinds = {"per_block": per_block, "verify_blocks": verify_blocks, "exec_blocks": exec_blocks}
        reps = max(3, -(-args.launches // nb))
        groups = -(-nb // 32)
        launches = {"per_block": nb, "verify_blocks": groups + 1, "exec_blocks": groups}  # per call
        graphs = {k: captured(torch, s, fn) for k, fn in kinds.items()}
        host = {k: [] for k in kinds}
        graph = {k: [] for k in kinds}
        for k, fn in kinds.items():  # steady state first: args.warmup launches of each kind, each way
            warm = max(2, -(-args.warmup // launches[k]))
            timed(torch, s, fn, warm)
            timed(torch, s, graphs[k].replay, warm)
        for _ in range(args.windows):  # alternating windows
            for k, fn in kinds.items():
                host[k].append(timed(torch, s, fn, reps))
            for k in kinds:
                graph[k].append(timed(torch, s, graphs[k].replay, reps))
        row = {"blocks": nb, "calls_per_window": reps, "verdicts_clean_ok": clean_ok, "verdicts_corrupted_ok": corrupt_ok}
        for k in kinds:
            row[k + "_host_issued"] = stats(host[k], nb)
            row[k + "_graph"] = stats(graph[k], nb)
        rows.append(row)
        graphs.clear()
        torch.cuda.synchronize()

    def first_win(mode):
        for r in rows:
            if r["verify_blocks_" + mode]["us"] < r["per_block_" + mode]["us"]:
                return r["blocks"]
        return None

    result = {"tool": "verify_blocks_rate", "device": torch.cuda.get_device_name(0), "block_bytes": BLOCK_BYTES,
              "bpc": BPC, "checksums_per_block": n, "windows": args.windows, "warmup_calls": args.warmup, "rows": rows,
              "smallest_blocks_where_verify_blocks_wins": {"host_issued": first_win("host_issued"),
                                                           "graph": first_win("graph")},
              "mismatches": bad}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    plan.close()
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
