"""Captured exec launches that may overlap (hdfs_crc32c.h section 3, "Captured
into a HIP graph"; csrc/crc32c_runtime.hip capture_exec): a captured
Plan.exec gets no edge from the previous captured exec of its context when
the two touch nothing in common, and keeps plain stream order in every other
case.  Every test replays its graph at least twice from poisoned outputs,
compares every checksum with the oracle, and asserts the context's counters
(execs captured, execs with no edge from their predecessor, runs started).

The batches are 16 MiB (256 packets of 64 KiB, 32768 checksums) unless a test
says otherwise: long enough launches that two of them overlap in time when an
edge is dropped that the result needed."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
NPAY = 4


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _extent(pk) -> int:
    return int((pk["payload_off"] + pk["len"]).max())


def _u32(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def _dev(torch, host: np.ndarray):
    """The bytes on the device, with 16 bytes of slack behind them."""
    t = torch.zeros(host.size + 16, dtype=torch.uint8, device="cuda")
    t[:host.size].copy_(torch.from_numpy(host))
    return t


def _outs(torch, n: int, count: int):
    return [torch.full((n,), POISON, dtype=torch.int32, device="cuda") for _ in range(count)]


@pytest.fixture(scope="module")
def rot(hdfs, orc):
    """Four 16 MiB payloads on the device and their checksums (shared, never
    written by a test)."""
    torch = _torch()
    pk = oracle.uniform_packets(256)
    n = hdfs.total_checksums(pk)
    host = [oracle.xorshift64_bytes(_extent(pk), 4100 + i) for i in range(NPAY)]
    return {"pk": pk, "n": n, "host": host, "dev": [_dev(torch, h) for h in host],
            "want": [orc.batch(h, pk, n) for h in host]}


def _capture(torch, body, mode="thread_local"):
    """Captures body(stream handle) on a fresh stream; mode None: torch's
    default (global) capture mode."""
    cs = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    kw = {} if mode is None else {"capture_error_mode": mode}
    with torch.cuda.graph(g, stream=cs, **kw):
        body(cs.cuda_stream)
    return g


def _replay(torch, g, reset, check, times: int = 2):
    for _ in range(times):
        reset()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check()


def _rotation(hdfs, torch, ctx, pk, devs, wants, mode="thread_local", nexec: int = 8):
    """nexec execs of one plan over len(devs) payloads into as many out
    arrays, captured and replayed twice; every array exact.  Returns the
    context's counters."""
    n = hdfs.total_checksums(pk)
    plan = ctx.plan(pk)
    outs = _outs(torch, n, len(devs))

    def body(s):
        for k in range(nexec):
            plan.exec(devs[k % len(devs)].data_ptr(), outs[k % len(devs)].data_ptr(), s)

    def reset():
        for o in outs:
            o.fill_(POISON)

    def check():
        for i, o in enumerate(outs):
            assert np.array_equal(_u32(o), wants[i]), i

    g = _capture(torch, body, mode)
    _replay(torch, g, reset, check)
    stats = ctx.capture_stats()
    del g
    plan.close()
    return stats


@pytest.mark.parametrize("mode", ["thread_local", None])
def test_independent_rotation(hdfs, rot, mode):
    """8 execs over 4 payloads into 4 out arrays: one run, every exec but the
    first without an edge from its predecessor (exec k follows exec k - 2,
    which wrote the array exec k + 2 writes again)."""
    torch = _torch()
    with hdfs.Context(0) as ctx:
        assert _rotation(hdfs, torch, ctx, rot["pk"], rot["dev"], rot["want"], mode) == (8, 7, 1)


def test_same_out_array(hdfs, rot):
    """12 execs alternating payloads A, B into ONE out array, ending on B:
    every exec keeps its edge and B's checksums are what every replay leaves."""
    torch = _torch()
    with hdfs.Context(0) as ctx:
        plan = ctx.plan(rot["pk"])
        out = _outs(torch, rot["n"], 1)[0]

        def body(s):
            for k in range(12):
                plan.exec(rot["dev"][k % 2].data_ptr(), out.data_ptr(), s)

        g = _capture(torch, body)
        _replay(torch, g, lambda: out.fill_(POISON), lambda: np.testing.assert_array_equal(_u32(out), rot["want"][1]),
                times=3)
        assert ctx.capture_stats() == (12, 0, 12)
        del g
        plan.close()


@pytest.mark.parametrize("order", ["read_after_write", "write_after_read"])
def test_exec_reads_what_another_writes(hdfs, orc, rot, order):
    """One exec writes its checksums into the head of a buffer X, the other
    checksums X itself: in either order they keep their edge.  Read after
    write: the second sees X with the first's checksums in its head; write
    after read: the first sees X as it was."""
    torch = _torch()
    pk, n = rot["pk"], rot["n"]
    x0 = oracle.xorshift64_bytes(_extent(pk), 4200)
    x1 = x0.copy()
    x1[:4 * n] = rot["want"][0].view(np.uint8)  # X after the writing exec (device byte order)
    want_x = orc.batch(x1 if order == "read_after_write" else x0, pk, n)
    x = _dev(torch, x0)
    x_init = x.clone()
    with hdfs.Context(0) as ctx:
        plan = ctx.plan(pk)
        out = _outs(torch, n, 1)[0]

        def write(s):
            plan.exec(rot["dev"][0].data_ptr(), x.data_ptr(), s)

        def read(s):
            plan.exec(x.data_ptr(), out.data_ptr(), s)

        def body(s):
            for f in ((write, read) if order == "read_after_write" else (read, write)):
                f(s)

        def reset():
            x.copy_(x_init)
            out.fill_(POISON)

        def check():
            assert np.array_equal(_u32(out), want_x)
            assert np.array_equal(x.cpu().numpy()[:x1.size], x1)

        g = _capture(torch, body)
        _replay(torch, g, reset, check, times=3)
        assert ctx.capture_stats() == (2, 0, 2)
        del g
        plan.close()


def test_foreign_node_between_execs(hdfs, orc, rot):
    """Between two otherwise independent execs, a captured copy into the
    second exec's payload on the same stream: the second exec starts a new
    run, follows the copy and checksums the copied bytes."""
    torch = _torch()
    pk, n = rot["pk"], rot["n"]
    dst = _dev(torch, oracle.xorshift64_bytes(_extent(pk), 4300))
    dst_init = dst.clone()
    src = rot["dev"][2]
    with hdfs.Context(0) as ctx:
        plan = ctx.plan(pk)
        outs = _outs(torch, n, 2)

        def body(s):
            plan.exec(rot["dev"][0].data_ptr(), outs[0].data_ptr(), s)
            dst.copy_(src)  # (on the capturing stream: a copy node)
            plan.exec(dst.data_ptr(), outs[1].data_ptr(), s)

        def reset():
            dst.copy_(dst_init)
            for o in outs:
                o.fill_(POISON)

        def check():
            assert np.array_equal(_u32(outs[0]), rot["want"][0])
            assert np.array_equal(_u32(outs[1]), rot["want"][2])

        g = _capture(torch, body)
        _replay(torch, g, reset, check, times=3)
        assert ctx.capture_stats() == (2, 0, 2)
        del g
        plan.close()


def test_exec_verify_exec_and_odd_end(hdfs, rot):
    """exec, verify, exec on one stream: the verify is clean, is not counted
    and ends the run (it is a node the execs did not put there); and a
    capture that ends right after an odd number of chained execs ends without
    error and replays exact."""
    torch = _torch()
    n = rot["n"]
    with hdfs.Context(0) as ctx:
        plan = ctx.plan(rot["pk"])
        outs = _outs(torch, n, 3)
        exp = torch.from_numpy(rot["want"][1].view(np.int32).copy()).cuda()
        res = torch.zeros(2, dtype=torch.int32, device="cuda")

        def body(s):
            plan.exec(rot["dev"][0].data_ptr(), outs[0].data_ptr(), s)
            plan.verify(rot["dev"][1].data_ptr(), exp.data_ptr(), res.data_ptr(), s)
            plan.exec(rot["dev"][2].data_ptr(), outs[2].data_ptr(), s)

        def reset():
            res.fill_(7)
            for o in outs:
                o.fill_(POISON)

        def check():
            assert _u32(res).tolist() == [0, 0xFFFFFFFF]
            assert np.array_equal(_u32(outs[0]), rot["want"][0])
            assert np.array_equal(_u32(outs[2]), rot["want"][2])

        g = _capture(torch, body)
        _replay(torch, g, reset, check)
        assert ctx.capture_stats() == (2, 0, 2)
        del g

        def odd(s):
            for k in range(3):
                plan.exec(rot["dev"][k].data_ptr(), outs[k].data_ptr(), s)

        def check3():
            for k in range(3):
                assert np.array_equal(_u32(outs[k]), rot["want"][k]), k

        g = _capture(torch, odd)
        _replay(torch, g, reset, check3)
        assert ctx.capture_stats() == (5, 2, 3)
        del g
        plan.close()


def test_two_plans_of_one_context(hdfs, orc, rot):
    """Two plans of one context (16 MiB at bpc 512, 4 MiB at bpc 1024)
    alternated over independent buffers share one run."""
    torch = _torch()
    pkb = oracle.uniform_packets(64, bpc=1024)
    nb = hdfs.total_checksums(pkb)
    want_b = [orc.batch(rot["host"][2 + i][:_extent(pkb)], pkb, nb) for i in range(2)]
    with hdfs.Context(0) as ctx:
        pa, pb = ctx.plan(rot["pk"]), ctx.plan(pkb)
        oa, ob = _outs(torch, rot["n"], 2), _outs(torch, nb, 2)

        def body(s):
            for k in range(8):
                i = (k // 2) % 2
                if k % 2 == 0:
                    pa.exec(rot["dev"][i].data_ptr(), oa[i].data_ptr(), s)
                else:
                    pb.exec(rot["dev"][2 + i].data_ptr(), ob[i].data_ptr(), s)

        def reset():
            for o in oa + ob:
                o.fill_(POISON)

        def check():
            for i in range(2):
                assert np.array_equal(_u32(oa[i]), rot["want"][i]), i
                assert np.array_equal(_u32(ob[i]), want_b[i]), i

        g = _capture(torch, body)
        _replay(torch, g, reset, check)
        assert ctx.capture_stats() == (8, 7, 1)
        del g
        pa.close()
        pb.close()


def test_ineligible_plans_stay_serial(hdfs, orc, rot):
    """Device-address plans and buffer-list plans (no single payload base of
    known extent) are counted and keep their edges; a pipelined multi plan's
    shard launches (its own exec streams) are not this feature's at all."""
    torch = _torch()
    blk = 64 * 65536  # one 4 MiB block: 64 packets, as crc32c_packetize cuts it
    pkb = oracle.uniform_packets(64)
    nb = hdfs.total_checksums(pkb)
    want = [orc.batch(rot["host"][i][:blk], pkb, nb) for i in range(NPAY)]
    with hdfs.Context(0) as ctx:
        plans = []
        for i in range(NPAY):
            if i % 2 == 0:
                pk = pkb.copy()
                pk["payload_off"] += np.uint64(rot["dev"][i].data_ptr())
                plans.append(hdfs.Plan(ctx, pk, hdfs.CRC32C_DEVICE_ADDRESSES))
            else:
                plans.append(ctx.write_plan([(rot["dev"][i].data_ptr(), blk)], 0, blk))
            assert plans[-1].nchecksums == nb
        outs = _outs(torch, nb, NPAY)

        def body(s):
            for k in range(2 * NPAY):
                plans[k % NPAY].exec(0, outs[k % NPAY].data_ptr(), s)

        def reset():
            for o in outs:
                o.fill_(POISON)

        def check():
            for i in range(NPAY):
                assert np.array_equal(_u32(outs[i]), want[i]), i

        g = _capture(torch, body)
        _replay(torch, g, reset, check)
        assert ctx.capture_stats() == (2 * NPAY, 0, 0)
        del g
        for p in plans:
            p.close()

    # the multi plan's pipelined capture (the shape of test_multi_plan_pipelined)
    gp, nfiles = 4, 4
    pk = oracle.uniform_packets(8 * gp)
    m = hdfs.Multi([0])
    mp = m.plan(pk, gp, hdfs.CRC32C_MULTI_PIPELINE)
    layout, sb = hdfs.multi_layout(pk, gp, 1)
    shards, wants = [], []
    for f in range(nfiles):
        payload = rot["host"][f][:_extent(pk)]
        host = np.zeros(int(sb[0]) + 16, np.uint8)
        for _, soff, poff, nbytes in layout.astype(np.int64):
            host[soff:soff + nbytes] = payload[poff:poff + nbytes]
        shards.append(torch.from_numpy(host).cuda())
        wants.append(orc.batch(payload, pk, mp.nchecksums))
    mouts = _outs(torch, mp.nchecksums, nfiles)
    cs = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs, capture_error_mode="thread_local"):
        for k in range(6):
            mp.exec([shards[k % nfiles].data_ptr()], mouts[k % nfiles].data_ptr(), [cs])
        mp.join([cs])

    def mreset():
        for o in mouts:
            o.fill_(POISON)

    def mcheck():
        for f in range(nfiles):
            assert np.array_equal(_u32(mouts[f]), wants[f]), f

    _replay(torch, g, mreset, mcheck)
    assert m.capture_stats()[1] == 0
    del g
    mp.close()
    m.close()


def test_switch_off(hdfs, rot):
    """Context.capture_overlap(False): the rotation keeps every edge."""
    torch = _torch()
    with hdfs.Context(0) as ctx:
        assert ctx.capture_overlap(False) is True
        assert _rotation(hdfs, torch, ctx, rot["pk"], rot["dev"], rot["want"]) == (8, 0, 0)
        assert ctx.capture_overlap(True) is False
        assert _rotation(hdfs, torch, ctx, rot["pk"], rot["dev"], rot["want"]) == (16, 7, 1)


_CHILD = """
import json, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import oracle
from conftest import load_package
import test_gpu_capture_chains as t
hdfs = load_package()
hdfs.lib()
orc = oracle.Oracle()
pk = oracle.uniform_packets(256)
n = hdfs.total_checksums(pk)
host = [oracle.xorshift64_bytes(t._extent(pk), 4100 + i) for i in range(t.NPAY)]
devs = [t._dev(torch, h) for h in host]
wants = [orc.batch(h, pk, n) for h in host]
with hdfs.Context(0) as ctx:
    print(json.dumps({"stats": t._rotation(hdfs, torch, ctx, pk, devs, wants)}))
"""


def test_switch_off_by_environment(hdfs, rot):
    """HDFS_CRC32C_CAPTURE_OVERLAP=0 in a fresh process: the same capture,
    every edge kept, results exact (asserted in the child)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HDFS_CRC32C_CAPTURE_OVERLAP="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(here), here)], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["stats"] == [8, 0, 0]


def test_smallest_launches(hdfs, orc, rot):
    """The rotation with one 64 KiB packet per launch (the quarter-unit
    build) and with one 5-byte packet (a single general-path item)."""
    torch = _torch()
    for pk in (oracle.uniform_packets(1), np.array([(0, 0, 5, 512)], hdfs.PACKET_DTYPE)):
        n = hdfs.total_checksums(pk)
        host = [rot["host"][i][1000:1000 + _extent(pk)].copy() for i in range(NPAY)]
        devs = [_dev(torch, h) for h in host]
        wants = [orc.batch(h, pk, n) for h in host]
        with hdfs.Context(0) as ctx:
            assert _rotation(hdfs, torch, ctx, pk, devs, wants) == (8, 7, 1)
