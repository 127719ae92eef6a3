"""Erasure coding on the GPU (include/hdfs_crc32c.h section 8; csrc/ec_rs.hip):
hdfs_ec_apply_dev and hdfs_ec_encode_striped_dev.  Expected bytes: the host
path hdfs_ec_apply (checked against the independent bitwise generator and the
stated pins in tests/test_ec_host.py) and the goldens (tests/golden/ec_rs.json).
All results are bit-exact.  In every test the outputs sit in a device buffer of
0xEE, and the WHOLE buffer is compared with its expected image, so every byte
outside the outputs must come back unchanged.  Sizes are placed from the
kernel's geometry hook."""
from __future__ import annotations

import errno
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0xEE


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X (cuda:0)"
    return torch


@pytest.fixture(scope="module")
def geom(hdfs):
    g = hdfs.debug_ec_geometry()
    assert g["lane_bytes"] == 16 and g["wave_bytes"] == 64 * g["lane_bytes"]
    assert g["workgroup_bytes"] == g["waves_per_workgroup"] * g["wave_bytes"]
    assert g["table_copies"] >= 32 and g["max_workgroups_per_cu"] >= 1
    assert g["lds_bytes_per_input"] == 32 * 4 * g["table_copies"] and 16 * g["lds_bytes_per_input"] <= g["lds_bytes_per_cu"]
    return g


@pytest.fixture(scope="module")
def data():
    d = oracle.xorshift64_bytes((1 << 20) + 4096, oracle.SEED)
    d.setflags(write=False)
    return d


class Dst:
    """A device buffer of 0xEE bytes (16-byte aligned) and its expected image on the host."""

    def __init__(self, nbytes: int):
        torch = _torch()
        self.t = torch.full((nbytes,), GUARD, dtype=torch.uint8, device="cuda")
        self.base = self.t.data_ptr()
        assert self.base % 16 == 0
        self.want = np.full(nbytes, GUARD, np.uint8)

    def expect(self, off: int, expected: np.ndarray) -> int:
        """Notes the bytes a call must leave at ``off``; returns the device address."""
        assert 0 <= off and off + expected.size <= self.want.size
        self.want[off:off + expected.size] = expected
        return self.base + off

    def reset(self):
        self.t.fill_(GUARD)
        self.want[:] = GUARD

    def check(self, what=""):
        _torch().cuda.synchronize()
        got = self.t.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, "%s: %d bytes differ, first at %d (got %02x, want %02x)" % (
            what, bad.size, bad[0], got[bad[0]], self.want[bad[0]])


class Units:
    """Input units in one device buffer: unit j is ``arrays[j]`` at offset offs[j] mod 16 of its own
    slot, with at least 16 bytes of slack each side (None stays None: a unit of zeros)."""

    def __init__(self, arrays, offs=None):
        torch = _torch()
        offs = offs or [0] * len(arrays)
        n = max([a.size for a in arrays if a is not None] + [0])
        self.pitch = (n + 63) // 16 * 16
        img = np.zeros(self.pitch * len(arrays) + 16, np.uint8)
        self.rel = []
        for j, (a, o) in enumerate(zip(arrays, offs)):
            self.rel.append(None if a is None else 16 + j * self.pitch + o)
            if a is not None:
                img[self.rel[-1]:self.rel[-1] + a.size] = a
        self.t = torch.from_numpy(img).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.addrs = [None if r is None else self.t.data_ptr() + r for r in self.rel]

    def update(self, arrays):
        torch = _torch()
        for r, a in zip(self.rel, arrays):
            if a is not None:
                self.t[r:r + a.size] = torch.from_numpy(np.array(a, copy=True)).cuda()


def apply_case(hdfs, ctx, mx, arrays, n, in_offs, out_offs, what, stream=0, before=None):
    """One hdfs_ec_apply_dev call over `n` bytes against hdfs_ec_apply, whole output buffer compared."""
    arrays = [None if a is None else a[:n] for a in arrays]
    units = Units(arrays, in_offs)
    pitch = (n + 63) // 16 * 16
    dst = Dst(pitch * mx.n_out + 32)
    want = mx.apply([np.zeros(n, np.uint8) if a is None else a for a in arrays])
    outs = [dst.expect(16 + r * pitch + out_offs[r], want[r]) for r in range(mx.n_out)]
    for r in range(mx.n_out):
        assert outs[r] % 16 == out_offs[r] % 16
    if before is not None:
        before()
    ctx.ec_apply(mx, units.addrs, outs, n, stream)
    dst.check(what)


def rand_matrix(hdfs, n_in, n_out, seed):
    rng = np.random.default_rng(seed)
    return hdfs.EcMatrix(rng.integers(1, 256, (n_out, n_in)).tolist())


def slices(data, count, n, step=4099):
    return [data[j * step:j * step + n] for j in range(count)]


# ---- 1. lengths --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["aligned", "odd"])
def test_lengths(hdfs, gpu_ctx, geom, data, mode):
    """RS(6,3) parity of units of 1, 15, 16, 17, 63, 4096 + 5 bytes, one wave unit -1 / 0 / +1 and one
    workgroup pass -1 / 0 / +1; everything aligned, and every pointer at its own odd phase."""
    mx = hdfs.EcMatrix.encode(6, 3)
    lens = [1, 15, 16, 17, 63, 4096 + 5] + [geom[u] + d for u in ("wave_bytes", "workgroup_bytes") for d in (-1, 0, 1)]
    in_offs = [0] * 6 if mode == "aligned" else [1, 7, 15, 4, 9, 10]
    out_offs = [0] * 3 if mode == "aligned" else [3, 14, 5]
    for n in lens:
        apply_case(hdfs, gpu_ctx, mx, slices(data, 6, n), n, in_offs, out_offs, "%d bytes (%s)" % (n, mode))


# ---- 2. the alignment cross ------------------------------------------------------------------
def _alignment_cases():
    cases = [([0] * 6, [0, 0, 0]), ([0] * 6, [0, 1, 0]), ([0] * 6, [1, 0, 0]), ([0] * 6, [0, 8, 4]), ([0] * 6, [0, 2, 6]),
             ([3] * 6, [3, 3, 3]), ([5, 0, 5, 0, 5, 0], [5, 13, 9]), ([2, 4, 6, 8, 10, 12], [7, 9, 15])]
    # every input and output at a different offset mod 16, through all 16 rotations
    cases += [([(s + j) % 16 for j in range(6)], [(s + 6 + 3 * r) % 16 for r in range(3)]) for s in range(16)]
    return cases


@pytest.mark.parametrize("half", [0, 1])
def test_alignment_cross(hdfs, gpu_ctx, geom, data, half):
    mx = hdfs.EcMatrix.encode(6, 3)
    n = 2 * geom["wave_bytes"] + 77
    cases = _alignment_cases()
    for in_offs, out_offs in cases[half::2]:
        apply_case(hdfs, gpu_ctx, mx, slices(data, 6, n), n, in_offs, out_offs, "in %s out %s" % (in_offs, out_offs))


# ---- 3. matrix shapes and NULL inputs ------------------------------------------------------------
@pytest.mark.parametrize("n_in", [1, 3, 6, 10, 16])
def test_matrix_shapes_and_null_inputs(hdfs, gpu_ctx, data, n_in):
    """n_in x n_out for n_out = 1 .. 4 with arbitrary coefficients; a NULL input in the first, a
    middle and the last position (n_in = 1: the only one)."""
    n = 1500
    for n_out in (1, 2, 3, 4):
        mx = rand_matrix(hdfs, n_in, n_out, 100 * n_in + n_out)
        arrays = slices(data, n_in, n)
        in_offs = [(3 * j + n_out) % 16 for j in range(n_in)]
        out_offs = [(11 * r) % 16 for r in range(n_out)]
        apply_case(hdfs, gpu_ctx, mx, arrays, n, in_offs, out_offs, "%d x %d" % (n_in, n_out))
        for absent in sorted({0, n_in // 2, n_in - 1}):
            holed = [None if j == absent else a for j, a in enumerate(arrays)]
            apply_case(hdfs, gpu_ctx, mx, holed, n, in_offs, out_offs, "%d x %d, input %d NULL" % (n_in, n_out, absent))


# ---- 4. the striped form ---------------------------------------------------------------------------
def host_striped_parity(hdfs, mx, buf, cell):
    """The parity blocks of a block group in file order, stripe by stripe on the host."""
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


@pytest.mark.parametrize("mode", ["aligned", "odd"])
def test_striped(hdfs, gpu_ctx, data, mode):
    """cell = 4096, k = 6: group lengths 1, cell, k cell, k cell + 1 and 3 k cell + 2 cell + 77; the
    parity bytes, and nothing written past each parity block's length."""
    torch = _torch()
    k, m, cell = 6, 3, 4096
    mx = hdfs.EcMatrix.encode(k, m)
    s_off, p_offs = (0, [0, 0, 0]) if mode == "aligned" else (5, [3, 12, 7])
    for length in (1, cell, k * cell, k * cell + 1, 3 * k * cell + 2 * cell + 77):
        buf = data[:length]
        src = torch.from_numpy(np.concatenate([np.zeros(16 + s_off, np.uint8), buf, np.zeros(32, np.uint8)])).cuda()
        par = host_striped_parity(hdfs, mx, buf, cell)
        pitch = (par[0].size + 2 * cell + 63) // 16 * 16  # (room for a wrongly full last stripe to show)
        dst = Dst(pitch * m + 32)
        outs = [dst.expect(16 + r * pitch + p_offs[r], par[r]) for r in range(m)]
        gpu_ctx.ec_encode_striped(mx, src.data_ptr() + 16 + s_off, length, cell, outs)
        dst.check("group of %d bytes (%s)" % (length, mode))


def test_striped_odd_cell(hdfs, gpu_ctx, data):
    """A cell that is no multiple of 16 (every stripe's parity at another phase), RS(3,2)."""
    torch = _torch()
    k, m, cell = 3, 2, 1000
    mx = hdfs.EcMatrix.encode(k, m)
    length = 4 * k * cell + cell + 123
    buf = data[:length]
    src = torch.from_numpy(np.concatenate([np.zeros(16 + 9, np.uint8), buf, np.zeros(32, np.uint8)])).cuda()
    par = host_striped_parity(hdfs, mx, buf, cell)
    pitch = (par[0].size + 2 * cell + 63) // 16 * 16
    dst = Dst(pitch * m + 32)
    outs = [dst.expect(16 + r * pitch + (2, 13)[r], par[r]) for r in range(m)]
    gpu_ctx.ec_encode_striped(mx, src.data_ptr() + 25, length, cell, outs)
    dst.check("cells of 1000 bytes")


def striped_src(buf, s_off, after=64):
    """A block group's bytes in device memory, s_off bytes past a 16-byte boundary, between bytes of 0xA5
    (a cell's end that is not masked shows: what follows the group is not zeros)."""
    torch = _torch()
    img = np.full(16 + s_off + buf.size + after, 0xA5, np.uint8)
    img[16 + s_off:16 + s_off + buf.size] = buf
    t = torch.from_numpy(img).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 16 + s_off


def striped_case(hdfs, ctx, mx, buf, cell, s_off, p_offs, what):
    """One hdfs_ec_encode_striped_dev call against host_striped_parity, whole output buffer compared."""
    src_t, src = striped_src(buf, s_off)
    par = host_striped_parity(hdfs, mx, buf, cell)
    pitch = (par[0].size + 2 * cell + 63) // 16 * 16  # (room for a wrongly full last stripe to show)
    dst = Dst(pitch * mx.n_out + 32)
    outs = [dst.expect(16 + r * pitch + p_offs[r], par[r]) for r in range(mx.n_out)]
    ctx.ec_encode_striped(mx, src, buf.size, cell, outs)
    dst.check(what)


@pytest.mark.parametrize("short", ["cell 1", "cell 2", "cell 0"])
def test_striped_last_cell_tails(hdfs, gpu_ctx, data, short):
    """RS(3,2), cells of 64 bytes, src 9 and the parities 2 and 13 bytes off a boundary: one full stripe,
    then a stripe whose cell 1 has t bytes behind a full cell 0, whose cell 2 has t bytes behind two full
    cells, and whose cell 0 itself has t bytes, for every t in 0 .. 33 -- every count of bytes the
    short-cell mask keeps in a word, at every word of a window and into a third window.  All calls read
    one source (bytes past a group's length are other data, not zeros) and write one buffer."""
    k, m, cell = 3, 2, 64
    mx = hdfs.EcMatrix.encode(k, m)
    full_cells = {"cell 0": 0, "cell 1": 1, "cell 2": 2}[short]
    tails = range(34)
    top = k * cell + full_cells * cell + max(tails)
    src_t, src = striped_src(data[100:100 + top + 40], 9, after=16)
    row = (2 * cell + 13 + 31) // 16 * 16
    dst = Dst(16 + len(tails) * m * row + 16)
    for t in tails:
        length = k * cell + full_cells * cell + t
        par = host_striped_parity(hdfs, mx, data[100:100 + length], cell)
        assert par[0].size == (cell + (cell if full_cells else t))
        outs = [dst.expect(16 + (t * m + r) * row + (2, 13)[r], par[r]) for r in range(m)]
        gpu_ctx.ec_encode_striped(mx, src, length, cell, outs)
    dst.check("short %s" % short)


@pytest.mark.parametrize("k,m", [(3, 2), (10, 4)])
def test_striped_small_and_odd_cells(hdfs, gpu_ctx, data, k, m):
    """Cells of 1, 2, 5, 15, 16, 17, 31 and 33 bytes (below 16: several stripes share one 16-byte window of
    a parity block), 5 stripes + 2 cells + half a cell, every pointer off a boundary."""
    mx = hdfs.EcMatrix.encode(k, m)
    for cell in (1, 2, 5, 15, 16, 17, 31, 33):
        length = 5 * k * cell + 2 * cell + cell // 2
        striped_case(hdfs, gpu_ctx, mx, data[cell:cell + length], cell, 9, [2, 13, 7, 5][:m],
                     "RS(%d,%d), cells of %d bytes" % (k, m, cell))


@pytest.mark.parametrize("mode", ["aligned", "odd"])
@pytest.mark.parametrize("scheme", ["rs-10-4", "xor-2-1", "16x4"])
def test_striped_schemes(hdfs, gpu_ctx, data, scheme, mode):
    """RS(10,4), XOR(2,1) and a 16 x 4 matrix of arbitrary coefficients over cells of 1024 + 16 bytes:
    groups of 1 byte, one cell, one stripe - 1 / 0 / + 1 and 3 stripes + 2 cells + 77."""
    mx = {"rs-10-4": lambda: hdfs.EcMatrix.encode(10, 4), "xor-2-1": lambda: hdfs.EcMatrix.encode(2, 1, hdfs.EC_XOR),
          "16x4": lambda: rand_matrix(hdfs, 16, 4, 164)}[scheme]()
    k, cell = mx.n_in, 1024 + 16
    s_off, p_offs = (0, [0, 0, 0, 0]) if mode == "aligned" else (5, [3, 12, 7, 9])
    for length in (1, cell, k * cell - 1, k * cell, k * cell + 1, 3 * k * cell + 2 * cell + 77):
        striped_case(hdfs, gpu_ctx, mx, data[:length], cell, s_off, p_offs[:mx.n_out],
                     "%s, group of %d bytes (%s)" % (scheme, length, mode))


def test_striped_beyond_one_pass_of_the_grid(hdfs, gpu_ctx, geom):
    """More wave units than waves in the launch, two per stripe: XOR(2,1) over cells of one wave unit with
    parity 0 three bytes past a boundary (a stripe's second unit holds one window of 3 bytes), and
    grid * waves_per_workgroup + 4 wave units -- the least even count that exceeds one pass by 3 or
    more -- so some waves take a second unit and divide it by units_per_stripe == 2.  The last stripe's
    cell 1 has 100 bytes.  Expected bytes: numpy's XOR of the cells."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    mx = hdfs.EcMatrix.encode(2, 1, hdfs.EC_XOR)
    assert mx.rows == [[1, 1]]
    cell = geom["wave_bytes"]
    per_cu = min(geom["max_workgroups_per_cu"], geom["lds_bytes_per_cu"] // (geom["lds_bytes_per_input"] * 2))
    one_pass = per_cu * cus * geom["waves_per_workgroup"]
    nstripes = (one_pass + 3 + 1) // 2
    assert 2 * nstripes >= one_pass + 3
    length = (nstripes - 1) * 2 * cell + cell + 100
    buf = oracle.xorshift64_bytes(length, oracle.SEED + 4)
    cells = np.concatenate([buf, np.zeros(cell - 100, np.uint8)]).reshape(nstripes, 2, cell)
    want = (cells[:, 0] ^ cells[:, 1]).reshape(-1)
    src_t, src = striped_src(buf, 6)
    dst = Dst(want.size + 2 * cell + 64)
    out = dst.expect(16 + 3, want)
    assert out % 16 == 3
    gpu_ctx.ec_encode_striped(mx, src, length, cell, [out])
    dst.check("%d stripes of two wave units" % nstripes)


# ---- 5. decode round trips -----------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,erased", [(6, 3, [0, 2, 5]), (10, 4, [1, 7, 10, 13])])
def test_decode_round_trip(hdfs, gpu_ctx, data, k, m, erased):
    """Encode on the GPU, lose units, rebuild them on the GPU from the first k survivors."""
    torch = _torch()
    n = 3000 + k
    enc = hdfs.EcMatrix.encode(k, m)
    arrays = slices(data, k, n)
    units = Units(arrays, [(5 * j) % 16 for j in range(k)])
    pitch = (n + 63) // 16 * 16
    par = Dst(pitch * m + 32)
    pouts = [par.expect(16 + r * pitch + r, w) for r, w in enumerate(enc.apply(arrays))]
    gpu_ctx.ec_apply(enc, units.addrs, pouts, n)
    par.check("parity")
    everything = units.addrs + pouts
    host = arrays + enc.apply(arrays)
    valid = [u for u in range(k + m) if u not in erased][:k]
    dec = hdfs.EcMatrix.decode(k, m, valid, erased)
    back = Dst(pitch * len(erased) + 32)
    bouts = [back.expect(16 + i * pitch + (7 * i) % 16, host[e]) for i, e in enumerate(erased)]
    gpu_ctx.ec_apply(dec, [everything[v] for v in valid], bouts, n)
    back.check("rebuilt units %s" % erased)
    torch.cuda.synchronize()


# ---- 6. goldens --------------------------------------------------------------------------------------
def test_goldens(hdfs, gpu_ctx):
    with open(os.path.join(GOLDEN, "ec_rs.json")) as f:
        golden = json.load(f)["schemes"]
    assert len(golden) == 4
    torch = _torch()
    for g in golden:
        k, m, n = g["k"], g["m"], g["unit_bytes"]
        t = np.arange(n, dtype=np.int64)
        units = Units([((31 * j + 7 * t + 1) & 0xff).astype(np.uint8) for j in range(k)])
        mx = hdfs.EcMatrix(np.frombuffer(bytes.fromhex("".join(g["parity_matrix"])), np.uint8).reshape(m, k).tolist())
        assert mx.rows == hdfs.EcMatrix.encode(k, m, hdfs.EC_XOR if g["codec"] == "xor" else hdfs.EC_RS).rows
        out = torch.full((m * n + 32,), GUARD, dtype=torch.uint8, device="cuda")
        gpu_ctx.ec_apply(mx, units.addrs, [out.data_ptr() + 16 + r * n for r in range(m)], n)
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert hashlib.sha256(h[16:-16].tobytes()).hexdigest() == g["parity_sha256"]
        assert [h[16 + r * n:32 + r * n].tobytes().hex() for r in range(m)] == g["parity_first16"]
        assert (h[:16] == GUARD).all() and (h[-16:] == GUARD).all()


# ---- 7. cold LDS ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0xC01DC0DE, 0x0DDBA11])
def test_cold_lds(hdfs, gpu_ctx, geom, data, seed):
    """The launch straight after every CU's LDS was poisoned, on the same stream: the tables are built
    from nothing an earlier launch left behind."""
    torch = _torch()
    mx = hdfs.EcMatrix.encode(10, 4)
    n = 4 * geom["workgroup_bytes"] + 5
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def poison():
        assert hdfs.debug_lds_poison(seed, s.cuda_stream) > 0

    apply_case(hdfs, gpu_ctx, mx, slices(data, 10, n, step=8191), n, [1] * 10, [3, 3, 3, 3], "after the poison",
               stream=s.cuda_stream, before=poison)


# ---- 8. graph replay --------------------------------------------------------------------------------------
def test_graph_replay(hdfs, gpu_ctx, data):
    """Both forms captured (the project's graphs.capture_agreed), replayed twice over changed inputs:
    the same calls, the same bytes."""
    from hdfs_crc32c_amd.graphs import capture_agreed

    torch = _torch()
    k, m, cell = 6, 3, 4096
    enc = hdfs.EcMatrix.encode(k, m)
    dec = hdfs.EcMatrix.decode(k, m, [0, 1, 3, 4, 6, 7], [2, 5])
    n = 5000
    length = 2 * k * cell + 3 * cell + 19
    units = Units(slices(data, k, n), [j for j in range(k)])
    src = torch.zeros(length + 64, dtype=torch.uint8, device="cuda")
    plen = hdfs.ec_group_layout(length, k, m, cell)[k]
    pitch_a, pitch_s = (n + 63) // 16 * 16, (plen + 63) // 16 * 16
    dst = Dst(2 * pitch_a + m * pitch_s + 64)
    a_outs = [dst.base + 16 + i * pitch_a + 5 * i for i in range(2)]
    s_outs = [dst.base + 16 + 2 * pitch_a + r * pitch_s + r for r in range(m)]
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()

    def capture():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            gpu_ctx.ec_apply(dec, units.addrs, a_outs, n, stream=cap.cuda_stream)
            gpu_ctx.ec_encode_striped(enc, src.data_ptr() + 16, length, cell, s_outs, stream=cap.cuda_stream)
        return g

    g, err = capture_agreed(capture, 1)
    assert g is not None, err
    for r in range(2):
        arrays = slices(data, k, n, step=4099 + 1000 * r)
        buf = data[777 * r:777 * r + length]
        units.update(arrays)
        src[16:16 + length] = torch.from_numpy(buf.copy()).cuda()
        dst.reset()
        for i, w in enumerate(dec.apply(arrays)):
            dst.expect(16 + i * pitch_a + 5 * i, w)
        for q, w in enumerate(host_striped_parity(hdfs, enc, buf, cell)):
            dst.expect(16 + 2 * pitch_a + q * pitch_s + q, w)
        torch.cuda.synchronize()
        g.replay()
        dst.check("replay %d" % r)
    del g


# ---- 9. the write order --------------------------------------------------------------------------------------
def test_write_order_encode_then_checksum(hdfs, gpu_ctx, orc, data):
    """An EC write on one stream with no host synchronisation in between: encode every stripe, then the
    nine internal blocks' plans (the data blocks where they lie in the file-order buffer, through
    hdfs_ec_block_packets).  The checksums are the oracle's over gathered host copies."""
    torch = _torch()
    k, m, cell, ps, bpc = 6, 3, 8192, 4096, 512
    enc = hdfs.EcMatrix.encode(k, m)
    length = 2 * k * cell + 4 * cell + 1000
    buf = data[:length]
    lens = hdfs.ec_group_layout(length, k, m, cell)
    par = host_striped_parity(hdfs, enc, buf, cell)
    src = torch.from_numpy(np.concatenate([buf, np.zeros(32, np.uint8)])).cuda()
    pitch = (lens[k] + 63) // 16 * 16
    dst = Dst(pitch * m + 32)
    pouts = [dst.expect(16 + r * pitch, par[r]) for r in range(m)]
    ncells = -(-length // cell)
    blocks = [np.concatenate([buf[i * cell:(i + 1) * cell] for i in range(b, ncells, k)]) for b in range(k)] + par
    pkts = [hdfs.ec_block_packets(length, k, cell, b, ps, bpc) for b in range(k)]
    ppk = oracle.uniform_packets(-(-lens[k] // ps), ps, bpc)
    ppk["len"][-1] = lens[k] - (len(ppk) - 1) * ps
    plans = [gpu_ctx.plan(pk) for pk in pkts] + [gpu_ctx.plan(ppk)]
    nsums = [hdfs.nchunks(n, bpc) for n in lens]
    sums = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in nsums]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu_ctx.ec_encode_striped(enc, src.data_ptr(), length, cell, pouts, stream=s.cuda_stream)
    for b in range(k):
        plans[b].exec(src.data_ptr(), sums[b].data_ptr(), s.cuda_stream)
    for r in range(m):
        plans[k].exec(pouts[r], sums[k + r].data_ptr(), s.cuda_stream)
    s.synchronize()
    dst.check("parity")
    for u in range(k + m):
        want = orc.chunks(np.ascontiguousarray(blocks[u]), bpc)
        assert blocks[u].size == lens[u]
        assert np.array_equal(sums[u].cpu().numpy().view(np.uint32), want), "internal block %d" % u
    for p in plans:
        p.close()


# ---- 10. the launch-size thresholds ------------------------------------------------------------------------------
def test_launch_size_thresholds(hdfs, gpu_ctx, geom):
    """A launch has at most (workgroups a CU holds for the matrix) * CUs workgroups: wave-unit counts of
    exactly that many (one wave per workgroup), one more (one workgroup runs a second wave),
    waves_per_workgroup times that many (every wave, one unit each) and one more (one wave loops),
    output 0 three bytes off; for a matrix of 2 inputs (the most workgroups per CU) and one of 16 (the
    fewest)."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = None
    for n_in in (2, 16):
        mx = hdfs.EcMatrix.encode(n_in, 1, hdfs.EC_XOR)
        per_cu = min(geom["max_workgroups_per_cu"], geom["lds_bytes_per_cu"] // (geom["lds_bytes_per_input"] * n_in))
        assert per_cu == (4 if n_in == 2 else 2)
        grid = per_cu * cus
        top = (grid * geom["waves_per_workgroup"] + 1) * geom["wave_bytes"]
        if big is None:
            big = oracle.xorshift64_bytes(top + 64 + 16 * 7, oracle.SEED + 2)
        for units in (grid, grid + 1, grid * geom["waves_per_workgroup"], grid * geom["waves_per_workgroup"] + 1):
            n = units * geom["wave_bytes"] - 3  # output 0 three bytes past a boundary: exactly `units` wave units
            apply_case(hdfs, gpu_ctx, mx, [big[7 * j:7 * j + n] for j in range(n_in)], n, [(6 + j) % 16 for j in range(n_in)],
                       [3], "%d inputs, %d wave units" % (n_in, units))


# ---- 11. argument errors ------------------------------------------------------------------------------------------
def test_argument_errors(hdfs, gpu_ctx, data):
    """Every refused call raises Crc32cError(-EINVAL) and launches nothing: the 0xEE buffers stay
    untouched.  Empty inputs succeed and write nothing."""
    mx = hdfs.EcMatrix.encode(3, 2)
    units = Units(slices(data, 3, 4096))
    i0, i1, i2 = units.addrs
    dst = Dst(3 * 8192)
    d = dst.base + 64
    closed = hdfs.Context.__new__(hdfs.Context)
    closed.handle, closed.device = None, 0

    def bad(n_in, n_out):
        b = hdfs.EcMatrix.encode(3, 2)
        b.c.n_in, b.c.n_out = n_in, n_out
        return b

    ap, st = gpu_ctx.ec_apply, gpu_ctx.ec_encode_striped
    AP, ST = "hdfs_ec_apply_dev", "hdfs_ec_encode_striped_dev"
    refused = [
        ("NULL ctx", AP, lambda: closed.ec_apply(mx, [i0, i1, i2], [d, d + 8192], 100)),
        ("NULL ctx (striped)", ST, lambda: closed.ec_encode_striped(mx, i0, 100, 16, [d, d + 8192])),
        ("NULL matrix", AP, lambda: ap(None, [i0, i1, i2], [d, d + 8192], 100)),
        ("NULL matrix (striped)", ST, lambda: st(None, i0, 100, 16, [d, d + 8192])),
        ("n_in == 0", AP, lambda: ap(bad(0, 2), [], [d, d + 8192], 100)),
        ("n_in == 17", AP, lambda: ap(bad(17, 2), [i0] * 17, [d, d + 8192], 100)),
        ("n_out == 0", AP, lambda: ap(bad(3, 0), [i0, i1, i2], [], 100)),
        ("n_out == 5", AP, lambda: ap(bad(3, 5), [i0, i1, i2], [d + 1024 * r for r in range(5)], 100)),
        ("a bad matrix (striped)", ST, lambda: st(bad(3, 5), i0, 100, 16, [d + 1024 * r for r in range(5)])),
        ("NULL input array", AP, lambda: ap(mx, None, [d, d + 8192], 100)),
        ("NULL output array", AP, lambda: ap(mx, [i0, i1, i2], None, 100)),
        ("NULL output", AP, lambda: ap(mx, [i0, i1, i2], [d, 0], 100)),
        ("an output over an input", AP, lambda: ap(mx, [i0, d + 8192 + 99, i2], [d, d + 8192], 100)),
        ("an output over an output", AP, lambda: ap(mx, [i0, i1, i2], [d, d + 99], 100)),
        ("cell == 0", ST, lambda: st(mx, i0, 100, 0, [d, d + 8192])),
        ("cell == 0, len == 0", ST, lambda: st(mx, i0, 0, 0, [d, d + 8192])),
        ("NULL src", ST, lambda: st(mx, 0, 100, 16, [d, d + 8192])),
        ("NULL parity array", ST, lambda: st(mx, i0, 100, 16, None)),
        ("NULL parity", ST, lambda: st(mx, i0, 100, 16, [0, d])),
        ("parity over src", ST, lambda: st(mx, d + 8192 + 10, 100, 16, [d, d + 8192])),
        ("parity over parity", ST, lambda: st(mx, i0, 100, 16, [d, d + 20])),
    ]
    for what, name, call in refused:
        with pytest.raises(hdfs.Crc32cError) as e:
            call()
        assert e.value.rc == -errno.EINVAL, what
        # the text is this call's own (the binding prefixes the entry point to crc32c_last_error's text,
        # which names it too), not one an earlier refused call left behind
        other = ST if name == AP else AP
        assert name + ": " + name + ": " in str(e.value) and other not in str(e.value), (what, str(e.value))
    # nothing to do: 0, nothing written, NULL pointers allowed
    ap(mx, None, None, 0)
    ap(mx, [0, 0, 0], [0, 0], 0)
    st(mx, 0, 0, 16, None)
    dst.check("after refused and empty calls")
    # all-NULL inputs are units of zeros
    dst.expect(64, np.zeros(100, np.uint8))
    dst.expect(64 + 8192, np.zeros(100, np.uint8))
    ap(mx, [None, None, None], [d, d + 8192], 100)
    dst.check("all inputs NULL")
