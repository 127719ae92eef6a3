"""Python view of libhdfs_crc32c.so -- the MI355X CRC32C chunk path of
native-hdfs-fuse, behind the C ABI in ``include/hdfs_crc32c.h``.

The reference is a C program; its interface for this path is the C function
``crc32c(crc, buf, len)`` (``src/crc32c.c:333``) called once per chunk by
``hadoop_rpc_send_packet`` (``src/hadooprpc.c:733-742``).  This module is a
thin ctypes mirror of the C ABI used by the tests and the bench; the product
is the shared library.  No CPU fallback exists for the GPU entry points: if
the library cannot reach a gfx950 device they raise ``Crc32cError``.

Device buffers are passed as raw pointers (``tensor.data_ptr()`` when the
caller uses torch for allocation) and streams as raw ``hipStream_t`` handles
(``torch.cuda.current_stream().cuda_stream``).
"""
from __future__ import annotations

import ctypes
import errno
import numbers
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libhdfs_crc32c.so")
DEBUG_LIB_PATH = os.path.join(HERE, "libhdfs_crc32c_debug.so")  # A/B variants + read probe (tools only)
INCLUDE_DIR = os.path.join(os.path.dirname(HERE), "include")

CRC32C_BIG_ENDIAN = 0x1
CRC32C_TYPE_CRC32 = 0x2  # Hadoop CHECKSUM_CRC32 (zlib polynomial) instead of CRC32C
CRC32C_DEVICE_ADDRESSES = 0x4  # plan flag: payload_off are device addresses; exec/verify take payload 0
CRC32C_CPU_FALLBACK = 0x8  # crc32c_chunks / crc32c_batch_host: finish on the host CPU if the GPU fails
CRC32C_MULTI_SELF_SEND = 0x10  # multi plan: rank 0's own checksums also go through RCCL (one-GPU transport test)
CRC32C_COUNT_COMPLETION = 0x20  # plan: launches count their completion on the GPU; destroy after the streams is safe
CRC32C_MULTI_PIPELINE = 0x40  # multi plan: consecutive execs overlap; results complete after join()
CRC32C_MULTI_PER_GROUP_RECV = 0x80  # multi plan (A/B): one send/recv pair per group range, no packed gather
CRC32C_VERIFY_OVERLAP = 0x80000000  # bit 31 of a verify result's count: overlapping verify launches
PATH_NONE, PATH_GPU, PATH_CPU = 0, 1, 2  # crc32c_last_path()

PACKET_DTYPE = np.dtype(
    [("payload_off", "<u8"), ("out_idx", "<u8"), ("len", "<u4"), ("bpc", "<u4")], align=True
)
TILE_DTYPE = np.dtype([("src", "<u8"), ("out", "<u4"), ("meta", "<u4")])
GEN_DTYPE = np.dtype([("src", "<u8"), ("out", "<u4"), ("len", "<u4")])
BUFFER_DTYPE = np.dtype([("data", "<u8"), ("len", "<u8")])  # crc32c_buffer (data 0 = zero fill)
FRAME_DTYPE = np.dtype([("frame_off", "<u8"), ("sums_off", "<u8"), ("data_off", "<u8"), ("offset_in_block", "<i8"),
                        ("seqno", "<i8"), ("data_len", "<u4"), ("nsums", "<u4"), ("last", "<u4"),
                        ("reserved", "<u4")])


class FramesResult(ctypes.Structure):
    _fields_ = [("packets", ctypes.c_uint64), ("data_bytes", ctypes.c_uint64), ("checksums", ctypes.c_uint64),
                ("mismatches", ctypes.c_uint64), ("first_bad", ctypes.c_uint64),
                ("first_bad_offset", ctypes.c_int64), ("consumed", ctypes.c_uint64),
                ("last_packet", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DebugBuild(ctypes.Structure):
    """crc32c_debug_build: hdfs_crc32c_plan_kernel<threads, waves_per_simd, mode> and its grid."""
    _fields_ = [("threads", ctypes.c_uint32), ("waves_per_simd", ctypes.c_uint32), ("mode", ctypes.c_uint32),
                ("units_per_tile", ctypes.c_uint32), ("grid", ctypes.c_uint32)]

    @property
    def kernel(self):
        return int(self.threads), int(self.waves_per_simd), int(self.mode)


class DebugLaunchInfo(ctypes.Structure):
    """crc32c_debug_launch_info: the KParams facts of a plan launch and the build chosen from them."""
    _fields_ = [("ntiles", ctypes.c_uint32), ("ngen", ctypes.c_uint32), ("nseg", ctypes.c_uint32),
                ("nconst", ctypes.c_uint32), ("general", ctypes.c_uint32), ("skip_z", ctypes.c_uint32),
                ("num_cu", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("build", DebugBuild)]


class DebugBlocksLaunch(ctypes.Structure):
    """crc32c_debug_blocks_launch: one launch of a multi-block call and the build chosen for it."""
    _fields_ = [("first_block", ctypes.c_uint32), ("nblocks", ctypes.c_uint32), ("ntiles", ctypes.c_uint32),
                ("general", ctypes.c_uint32), ("skip_z", ctypes.c_uint32), ("num_cu", ctypes.c_uint32),
                ("per_block", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("build", DebugBuild)]


class DebugAesLaunch(ctypes.Structure):
    """crc32c_debug_aes_launch: the sizing of one AES/CTR launch."""
    _fields_ = [("windows", ctypes.c_uint64), ("wave_units", ctypes.c_uint64),
                ("windows_per_lane", ctypes.c_uint32), ("grid", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class Crc32cError(RuntimeError):
    def __init__(self, rc: int, msg: str):
        super().__init__("%s (rc=%d %s)" % (msg, rc, errno.errorcode.get(-rc, "?")))
        self.rc = rc


def build(quiet: bool = True) -> str:
    """Compile the library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.DEVNULL if quiet else None
    jobs = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-C", HERE, "-j" + jobs], check=True, stdout=out)
    return LIB_PATH


_LIB = None
_DEBUG_LIB = None


def lib():
    """Load (not build) the shared library; raises if it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(LIB_PATH + " is not built (run build())")
        # One HIP runtime per process: torch ships its own libamdhip64 and
        # librccl and links them by the unversioned names, so it must be
        # loaded first; our NEEDED libamdhip64.so.7 / librccl.so.1 then bind
        # to the same copies by SONAME.  (Loaded the other way round the
        # process would hold two runtimes and torch would see no device.)
        # torch is plumbing only (device memory, streams, torch.distributed);
        # nothing here computes with it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _LIB = _bind(ctypes.CDLL(LIB_PATH))
    return _LIB


def debug_lib():
    """libhdfs_crc32c_debug.so (A/B kernel variants, HBM read probe); it links
    against the product library, which is loaded first."""
    global _DEBUG_LIB
    if _DEBUG_LIB is None:
        lib()
        if not os.path.exists(DEBUG_LIB_PATH):
            raise FileNotFoundError(DEBUG_LIB_PATH + " is not built (run build())")
        L = ctypes.CDLL(DEBUG_LIB_PATH)
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        L.crc32c_debug_plan_exec_variant.restype = i32
        L.crc32c_debug_plan_exec_variant.argtypes = [vp, vp, vp, vp, i32, vp]
        L.crc32c_debug_stream_probe.restype = i32
        L.crc32c_debug_stream_probe.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint32, i32, vp]
        L.crc32c_debug_variant_name.restype = ctypes.c_char_p
        L.crc32c_debug_variant_name.argtypes = [i32, ctypes.POINTER(i32)]
        L.crc32c_debug_lds_poison.restype = i32
        L.crc32c_debug_lds_poison.argtypes = [ctypes.c_uint32, vp]
        L.crc32c_debug_lds_peek.restype = i32
        L.crc32c_debug_lds_peek.argtypes = [ctypes.c_uint32, vp, vp]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        for name, args in (("crc32c_debug_resident_create", [vp, ctypes.c_uint32, ctypes.POINTER(vp)]),
                           ("crc32c_debug_resident_submit", [vp, vp, vp, u64p]),
                           ("crc32c_debug_resident_wait", [vp, ctypes.c_uint64]),
                           ("crc32c_debug_resident_stats", [vp, u64p]),
                           ("crc32c_debug_resident_destroy", [vp])):
            f = getattr(L, name)
            f.restype = i32
            f.argtypes = args
        _DEBUG_LIB = L
    return _DEBUG_LIB


class Resident:
    """crc32c_debug_resident_* (debug library, A/B experiment): a resident
    kernel taking one block's plan over blocks submitted by any thread."""

    def __init__(self, plan: "Plan", idle_us: int = 0):
        h = ctypes.c_void_p()
        L = debug_lib()
        _check(L.crc32c_debug_resident_create(plan.handle, idle_us, ctypes.byref(h)), "crc32c_debug_resident_create")
        self.plan = plan  # (outlives the resident kernel)
        self.handle = h

    def submit(self, dev_payload: int, dev_out: int) -> int:
        t = ctypes.c_uint64(0)
        _check(debug_lib().crc32c_debug_resident_submit(self.handle, ctypes.c_void_p(dev_payload),
                                                        ctypes.c_void_p(dev_out), ctypes.byref(t)),
               "crc32c_debug_resident_submit")
        return int(t.value)

    def wait(self, ticket: int) -> None:
        _check(debug_lib().crc32c_debug_resident_wait(self.handle, ticket), "crc32c_debug_resident_wait")

    def launches(self) -> int:
        n = ctypes.c_uint64(0)
        _check(debug_lib().crc32c_debug_resident_stats(self.handle, ctypes.byref(n)), "crc32c_debug_resident_stats")
        return int(n.value)

    def close(self) -> None:
        if self.handle:
            debug_lib().crc32c_debug_resident_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_lds_poison(seed: int, stream=0) -> int:
    """crc32c_debug_lds_poison (debug library): every CU's LDS filled with the seed's
    pattern by a launch on ``stream``; returns the workgroups launched."""
    n = int(debug_lib().crc32c_debug_lds_poison(seed & 0xFFFFFFFF, ctypes.c_void_p(_stream_handle(stream, {}))))
    if n < 0:
        _check(n, "crc32c_debug_lds_poison")
    return n


def debug_lds_peek(seed: int, dev_counts: int = 0, stream=0) -> int:
    """crc32c_debug_lds_peek (debug library): per workgroup, the LDS words still holding the
    seed's pattern, into dev_counts (u32 each); returns the workgroups (dev_counts 0: only that)."""
    n = int(debug_lib().crc32c_debug_lds_peek(seed & 0xFFFFFFFF, ctypes.c_void_p(dev_counts),
                                              ctypes.c_void_p(_stream_handle(stream, {}))))
    if n < 0:
        _check(n, "crc32c_debug_lds_peek")
    return n


def variant_info(v: int):
    """(name, exact) of a kernel variant built into the debug library, or None."""
    ex = ctypes.c_int(0)
    name = debug_lib().crc32c_debug_variant_name(v, ctypes.byref(ex))
    return None if name is None else (name.decode(), bool(ex.value))


def _bind(L):
    u32, u64, i32, vp, sz = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    pp = ctypes.POINTER(vp)
    sig = {
        "crc32c": (u32, [u32, vp, sz]),
        "crc32c_nchunks": (u64, [u64, u32]),
        "crc32c_packetize": (u64, [u64, u64, u32, u32, vp, u64]),
        "crc32c_batch_nchecksums": (u64, [vp, sz]),
        "crc32c_chunks_cpu": (i32, [vp, sz, u32, vp, u32]),
        "crc32c_device_count": (i32, []),
        "crc32c_ctx_create": (i32, [i32, pp]),
        "crc32c_ctx_destroy": (i32, [vp]),
        "crc32c_ctx_capture_overlap": (i32, [vp, i32]),
        "crc32c_ctx_capture_stats": (i32, [vp, ctypes.POINTER(u64)]),
        "crc32c_debug_multi_capture_stats": (i32, [vp, i32, ctypes.POINTER(u64)]),
        "crc32c_plan_create": (i32, [vp, vp, sz, u32, pp]),
        "crc32c_plan_exec": (i32, [vp, vp, vp, vp]),
        "crc32c_plan_destroy": (i32, [vp]),
        "crc32c_plan_nchecksums": (u64, [vp]),
        "crc32c_plan_payload_bytes": (u64, [vp]),
        "crc32c_chunks_dev": (i32, [vp, vp, sz, vp, vp, u32, vp]),
        "crc32c_batch_host": (i32, [vp, vp, vp, sz, vp, u32]),
        "crc32c_chunks": (i32, [vp, sz, u32, vp, u32]),
        "crc32c_multi_create": (i32, [vp, i32, pp]),
        "crc32c_multi_destroy": (i32, [vp]),
        "crc32c_multi_batch_host": (i32, [vp, vp, vp, sz, u32, vp, u32]),
        "crc32c_last_error": (ctypes.c_char_p, []),
        "crc32c_debug_plan": (i32, [vp, sz, vp, sz, vp, sz, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "crc32c_debug_plan_abs": (i32, [vp, sz, i32, vp, sz, vp, sz, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "crc32c_debug_lds_image": (sz, [vp, sz, vp, vp]),
        "crc32c_debug_lds_image_s4": (sz, [vp, sz, u32]),
        "crc32c_debug_lds_image_s4_split": (sz, [vp, sz, u32]),
        "crc32c_plan_verify": (i32, [vp, vp, vp, vp, vp]),
        "crc32c_plan_verify_bitmap": (i32, [vp, vp, vp, vp, vp, vp]),
        "crc32c_frame_packets": (sz, [vp, sz, vp, u32, u64, ctypes.c_int64, u32, vp, sz, vp]),
        "crc32c_block_md5": (None, [vp, sz, u32, vp]),
        "crc32c_md5_nblocks": (u64, [u64, u32]),
        "crc32c_md5_blocks": (i32, [vp, vp, u64, u32, u32, vp, vp]),
        "crc32c_md5_block_list": (i32, [vp, vp, vp, sz, u32, vp, vp]),
        "crc32c_plan_exec_blocks_md5": (i32, [vp, vp, vp, sz, vp, vp]),
        "crc32c_file_md5": (None, [vp, sz, vp]),
        "crc32c_combine": (u32, [u32, u32, u64, u32]),
        "crc32c_block_composite": (i32, [vp, sz, u32, u32, u32, vp]),
        "crc32c_file_composite": (i32, [vp, vp, sz, u32, vp]),
        "crc32c_composite_cells": (i32, [vp, vp, u64, u32, u32, u32, u32, vp, vp]),
        "crc32c_composite_block_list": (i32, [vp, vp, vp, vp, sz, u32, u32, vp, vp]),
        "crc32c_plan_exec_blocks_composite": (i32, [vp, vp, vp, sz, vp, vp]),
        "crc32c_plan_composite_shape": (i32, [vp, vp, vp]),
        "crc32c_debug_composite_geometry": (None, [vp]),
        "crc32c_debug_packets_composite_shape": (i32, [vp, sz, vp, vp]),
        "crc32c_bitmap_verdicts_host": (i32, [vp, u64, u32, vp]),
        "crc32c_bitmap_verdicts": (i32, [vp, vp, u64, u32, vp, vp]),
        "crc32c_plan_verify_blocks_work_bytes": (u64, [vp, sz]),
        "crc32c_plan_verify_blocks": (i32, [vp, vp, vp, sz, vp, vp, vp]),
        "crc32c_debug_verdict_geometry": (None, [vp]),
        "crc32c_verify_host": (ctypes.c_int64, [vp, vp, vp, sz, vp, u32, vp]),
        "crc32c_debug_affine_constants": (None, [u32, vp, vp]),
        "hdfs_crc32": (u32, [u32, vp, sz]),
        "crc32c_last_path": (i32, []),
        "crc32c_plan_create_buffers": (i32, [vp, vp, u32, u64, u64, u64, u32, u32, u32, pp]),
        "crc32c_debug_write_plan": (i32, [vp, u32, u64, u64, u64, u32, u32, vp]),
        "crc32c_multi_unique_id": (i32, [vp]),
        "crc32c_multi_create_rank": (i32, [i32, i32, i32, vp, pp]),
        "crc32c_multi_sync": (i32, [vp]),
        "crc32c_multi_layout": (ctypes.c_int64, [vp, sz, u32, i32, vp, vp]),
        "crc32c_multi_shard_packets": (ctypes.c_int64, [vp, sz, u32, i32, i32, vp, sz]),
        "crc32c_multi_rank_packets": (ctypes.c_int64, [vp, sz, u32, i32, i32, u32, vp, sz]),
        "crc32c_multi_transfers": (ctypes.c_int64, [vp, sz, u32, i32, u32, vp, vp, sz]),
        "crc32c_multi_scatter": (ctypes.c_int64, [vp, sz, u32, i32, u32, vp, vp, sz]),
        "crc32c_multi_plan_create": (i32, [vp, vp, sz, u32, u32, pp]),
        "crc32c_multi_plan_exec": (i32, [vp, vp, vp, vp]),
        "crc32c_multi_plan_join": (i32, [vp, vp]),
        "crc32c_multi_plan_destroy": (i32, [vp]),
        "crc32c_multi_plan_nchecksums": (u64, [vp]),
        "crc32c_multi_plan_shard_bytes": (u64, [vp, i32]),
        "crc32c_multi_plan_gather_ops": (u64, [vp, ctypes.POINTER(ctypes.c_int)]),
        "crc32c_parse_frames": (ctypes.c_int64, [vp, sz, vp, sz, ctypes.POINTER(u64)]),
        "crc32c_plan_exec_blocks": (i32, [vp, vp, vp, sz, vp]),
        "crc32c_blocks_create": (i32, [vp, u32, u32, pp]),
        "crc32c_block_submit": (i32, [vp, vp, vp, ctypes.POINTER(u64)]),
        "crc32c_block_submit_plan": (i32, [vp, vp, vp, vp, ctypes.POINTER(u64)]),
        "crc32c_block_flush": (i32, [vp]),
        "crc32c_block_wait": (i32, [vp, u64]),
        "crc32c_block_checksums": (i32, [vp, vp, vp]),
        "crc32c_blocks_stats": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "crc32c_blocks_destroy": (i32, [vp]),
        "crc32c_blocks_create_resident": (i32, [vp, u32, pp]),
        "crc32c_debug_plan_block": (u64, [vp]),
        "crc32c_debug_blocks_fail_flushes": (i32, [vp, u32]),
        "crc32c_debug_blocks_resident_inject": (i32, [vp, i32, u32]),
        "crc32c_verify_frames_host": (i32, [vp, vp, sz, u32, u64, u32, ctypes.POINTER(FramesResult)]),
        "crc32c_debug_select_build": (i32, [u32, u32, u32, u32, u32, i32, u32, ctypes.POINTER(DebugBuild)]),
        "crc32c_debug_plan_launch_info": (i32, [vp, vp, i32, ctypes.POINTER(DebugLaunchInfo)]),
        "crc32c_debug_plan_blocks_launch_info": (i32, [vp, vp, vp, sz, i32, vp, sz]),
        "crc32c_debug_packets_flags": (i32, [vp, sz, i32, ctypes.POINTER(u32), ctypes.POINTER(i32)]),
        "hdfs_aes_ctr_init": (i32, [vp, vp, u32, vp]),
        "hdfs_aes_ctr_counter": (None, [vp, u64, vp]),
        "hdfs_aes_ctr_xor": (i32, [vp, u64, vp, vp, sz]),
        "hdfs_aes_ctr_xor_strided_dev": (i32, [vp, vp, vp, vp, u64, u64, u64, u64, u64, u64, vp]),
        "hdfs_aes_ctr_xor_list_dev": (i32, [vp, vp, vp, sz, vp]),
        "hdfs_aes_wire_segments": (ctypes.c_int64, [vp, sz, vp, u64, vp, vp, vp, vp, sz]),
        "crc32c_debug_aes_geometry": (None, [vp]),
        "crc32c_debug_aes_strided_launch_info": (i32, [u32, vp, u64, u64, u64, ctypes.POINTER(DebugAesLaunch)]),
        "crc32c_debug_aes_list_launch_info": (i32, [u32, vp, sz, ctypes.POINTER(DebugAesLaunch)]),
        "hdfs_gf256_mul": (ctypes.c_uint8, [ctypes.c_uint8, ctypes.c_uint8]),
        "hdfs_gf256_inv": (ctypes.c_uint8, [ctypes.c_uint8]),
        "hdfs_ec_encode_matrix": (i32, [i32, u32, u32, vp]),
        "hdfs_ec_decode_matrix": (i32, [i32, u32, u32, vp, vp, u32, vp]),
        "hdfs_ec_group_layout": (i32, [u64, u32, u32, u64, vp]),
        "hdfs_ec_block_packets": (ctypes.c_int64, [u64, u32, u64, u32, u32, u32, u64, vp, sz]),
        "hdfs_ec_apply": (i32, [vp, vp, vp, sz]),
        "hdfs_ec_apply_dev": (i32, [vp, vp, vp, vp, u64, vp]),
        "hdfs_ec_encode_striped_dev": (i32, [vp, vp, vp, u64, u64, vp, vp]),
        "crc32c_debug_ec_geometry": (None, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise Crc32cError(rc, "%s: %s" % (what, lib().crc32c_last_error().decode(errors="replace")))


def _np_ptr(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def _stream_handle(stream, keep: dict) -> int:
    """A raw hipStream_t handle from a handle (int, numpy integer, None = the
    default stream) or a stream object (``.cuda_stream``, e.g. a
    ``torch.cuda.Stream``); a stream object is kept alive in ``keep`` (the
    library touches a plan's launch streams until the plan is destroyed)."""
    if stream is None:
        return 0
    if isinstance(stream, numbers.Integral):
        return int(stream)
    h = int(stream.cuda_stream)
    keep.setdefault(h, stream)
    return h


def as_packets(pkts) -> np.ndarray:
    return np.ascontiguousarray(pkts, dtype=PACKET_DTYPE)


# --- 1. drop-in scalar (host CPU, identical to src/crc32c.c:333) ----------
def crc32c(data, crc: int = 0) -> int:
    a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data)
    return int(lib().crc32c(crc & 0xFFFFFFFF, _np_ptr(a), a.nbytes))


def hdfs_crc32(data, crc: int = 0) -> int:
    """Hadoop CHECKSUM_CRC32 on the host (zlib-compatible crc32)."""
    a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data)
    return int(lib().hdfs_crc32(crc & 0xFFFFFFFF, _np_ptr(a), a.nbytes))


def frame_packets(pkts, sums: np.ndarray, flags: int = 0, block_offset: int = 0, first_seqno: int = 0,
                  checksum_len: int = 4):
    """Per-packet send prefixes (PLEN | HLEN | PacketHeaderProto | checksums) of
    a batch: (bytes, offsets[npkts + 1])."""
    pkts = as_packets(pkts)
    sums = np.ascontiguousarray(sums, dtype=np.uint32)
    need = int(lib().crc32c_frame_packets(_np_ptr(pkts), pkts.size, _np_ptr(sums), flags, block_offset,
                                          first_seqno, checksum_len, None, 0, None))
    out = np.zeros(max(need, 1), np.uint8)
    offs = np.zeros(pkts.size + 1, np.uint64)
    got = int(lib().crc32c_frame_packets(_np_ptr(pkts), pkts.size, _np_ptr(sums), flags, block_offset,
                                         first_seqno, checksum_len, _np_ptr(out), out.size, _np_ptr(offs)))
    if got != need:
        raise Crc32cError(-errno.EINVAL, "crc32c_frame_packets")
    return out[:need].tobytes(), offs


def block_md5(sums: np.ndarray, flags: int = 0) -> bytes:
    """OpBlockChecksumResponseProto.md5 of a block's checksums."""
    sums = np.ascontiguousarray(sums, dtype=np.uint32)
    md5 = np.zeros(16, np.uint8)
    lib().crc32c_block_md5(_np_ptr(sums), sums.size, flags, _np_ptr(md5))
    return md5.tobytes()


MD5_LIST_MAX_BLOCKS = 256  # CRC32C_MD5_LIST_MAX_BLOCKS: blocks per launch of Context.md5_block_list


def md5_nblocks(nsums: int, crc_per_block: int) -> int:
    """Blocks (digests) of a contiguous checksum array cut every crc_per_block checksums."""
    return int(lib().crc32c_md5_nblocks(nsums, crc_per_block))


def file_md5(block_md5s) -> bytes:
    """crc32c_file_md5: MD5 over the concatenated 16-byte block digests (bytes, or a
    uint8 array of 16 n bytes) = Hadoop's MD5-of-MD5-of-CRC file checksum."""
    a = np.frombuffer(bytes(block_md5s), np.uint8) if not isinstance(block_md5s, np.ndarray) else block_md5s
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    if a.size % 16:
        raise ValueError("block digests are 16 bytes each (%d bytes given)" % a.size)
    md5 = np.zeros(16, np.uint8)
    lib().crc32c_file_md5(_np_ptr(a) if a.size else None, a.size // 16, _np_ptr(md5))
    return md5.tobytes()


COMPOSITE_LIST_MAX_BLOCKS = 240  # CRC32C_COMPOSITE_LIST_MAX_BLOCKS: blocks per launch of Context.composite_block_list


def combine(crc_a: int, crc_b: int, len_b: int, flags: int = 0) -> int:
    """crc32c_combine: the CRC of A || B from crc(A), crc(B) and len(B) (flags: CRC32C_TYPE_CRC32)."""
    return int(lib().crc32c_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, len_b, flags))


def block_composite(sums: np.ndarray, bpc: int, last_len: int, flags: int = 0) -> int:
    """crc32c_block_composite: chunk checksums (stored in host order, or wire order with
    CRC32C_BIG_ENDIAN) -> the CRC of the bytes they cover; every chunk after the first is bpc bytes
    long, the last one last_len."""
    sums = np.ascontiguousarray(sums, dtype=np.uint32)
    crc = ctypes.c_uint32(0)
    _check(lib().crc32c_block_composite(_np_ptr(sums) if sums.size else None, sums.size, bpc, last_len, flags,
                                        ctypes.byref(crc)), "crc32c_block_composite")
    return int(crc.value)


def file_composite(block_crcs, block_lens, flags: int = 0) -> int:
    """crc32c_file_composite: block CRCs (host order) combined by the blocks' byte lengths = the
    value of Hadoop's COMPOSITE-CRC32C / COMPOSITE-CRC32 file checksum (wire form: 4 big-endian bytes)."""
    crcs = np.ascontiguousarray(block_crcs, dtype=np.uint32).reshape(-1)
    lens = np.ascontiguousarray(block_lens, dtype=np.uint64).reshape(-1)
    if crcs.size != lens.size:
        raise ValueError("block_crcs and block_lens differ in length")
    crc = ctypes.c_uint32(0)
    _check(lib().crc32c_file_composite(_np_ptr(crcs) if crcs.size else None, _np_ptr(lens) if lens.size else None,
                                       crcs.size, flags, ctypes.byref(crc)), "crc32c_file_composite")
    return int(crc.value)


def debug_composite_geometry() -> dict:
    """crc32c_debug_composite_geometry: the composite kernel's run, lanes, waves_per_workgroup, split_above."""
    g = np.zeros(4, np.uint32)
    lib().crc32c_debug_composite_geometry(_np_ptr(g))
    return dict(zip(["run", "lanes", "waves_per_workgroup", "split_above"], (int(x) for x in g)))


# crc32c_block_verdict: one per cell of a mismatch bitmap / per block of Plan.verify_blocks
BLOCK_VERDICT_DTYPE = np.dtype([("mismatches", "<u4"), ("first_bad", "<u4"), ("last_bad", "<u4"), ("reserved", "<u4")])


def bitmap_verdicts_host(bits: np.ndarray, nsums: int, crc_per_cell: int) -> np.ndarray:
    """crc32c_bitmap_verdicts_host: a mismatch bitmap in host memory (u32 words, bit k = bit k % 32 of
    word k // 32) cut into cells of crc_per_cell bits -> one BLOCK_VERDICT_DTYPE record per cell (count,
    lowest and highest set bit counted from the cell's first bit, 0xffffffff when none)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    ncells = md5_nblocks(nsums, crc_per_cell)
    out = np.zeros(max(ncells, 1), BLOCK_VERDICT_DTYPE)
    _check(lib().crc32c_bitmap_verdicts_host(_np_ptr(bits) if bits.size else None, nsums, crc_per_cell,
                                             _np_ptr(out)), "crc32c_bitmap_verdicts_host")
    return out[:ncells]


def debug_verdict_geometry() -> dict:
    """crc32c_debug_verdict_geometry: the verdict kernel's lane_max_cell, lanes, waves_per_workgroup, grid_cap."""
    g = np.zeros(4, np.uint32)
    lib().crc32c_debug_verdict_geometry(_np_ptr(g))
    return dict(zip(["lane_max_cell", "lanes", "waves_per_workgroup", "grid_cap"], (int(x) for x in g)))


# --- 7. AES/CTR/NoPadding (encrypted transfer, encryption zones) -----------
AES_LIST_MAX_SEGMENTS = 64  # HDFS_AES_LIST_MAX_SEGMENTS: segments per launch of Context.aes_ctr_xor_list
# hdfs_aes_segment: src / dst device addresses (0 allowed where len == 0)
AES_SEGMENT_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("stream_off", "<u8"), ("len", "<u8")])


class _AesCtrStruct(ctypes.Structure):
    _fields_ = [("rk", ctypes.c_uint32 * 60), ("iv", ctypes.c_uint8 * 16), ("rounds", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 3)]


class AesCtr:
    """hdfs_aes_ctr: an expanded AES key (16, 24 or 32 bytes) and a 16-byte IV.  ``xor`` is the host
    path (encrypting and decrypting are the same call); the device forms are
    ``Context.aes_ctr_xor_strided`` and ``Context.aes_ctr_xor_list``."""

    def __init__(self, key: bytes, iv: bytes):
        self.c = _AesCtrStruct()
        self.init(key, iv)

    def init(self, key: bytes, iv: bytes) -> None:
        key, iv = bytes(key), bytes(iv)
        if len(iv) != 16:
            raise ValueError("the IV is 16 bytes (%d given)" % len(iv))
        kb = (ctypes.c_uint8 * max(len(key), 1)).from_buffer_copy(key or b"\0")
        ib = (ctypes.c_uint8 * 16).from_buffer_copy(iv)
        _check(lib().hdfs_aes_ctr_init(ctypes.byref(self.c), kb, 8 * len(key), ib), "hdfs_aes_ctr_init")

    @property
    def rounds(self) -> int:
        return int(self.c.rounds)

    @property
    def handle(self):
        return ctypes.byref(self.c)

    @staticmethod
    def counter(iv: bytes, block_index: int) -> bytes:
        """hdfs_aes_ctr_counter: ctr(block_index) = IV + block_index, 128-bit big-endian (calculateIV)."""
        ib = (ctypes.c_uint8 * 16).from_buffer_copy(bytes(iv))
        out = (ctypes.c_uint8 * 16)()
        lib().hdfs_aes_ctr_counter(ib, block_index, out)
        return bytes(out)

    def xor(self, stream_off: int, data, out: np.ndarray | None = None) -> np.ndarray:
        """hdfs_aes_ctr_xor: data ^ keystream(stream_off ...) on the host.  ``data`` is bytes or a
        uint8 array (views at any alignment are used where they lie); ``out`` (optional, may be
        ``data`` itself) receives the result."""
        a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
        if a.dtype != np.uint8 or (a.size and not a.flags.c_contiguous):
            a = np.ascontiguousarray(a, dtype=np.uint8)
        if out is None:
            out = np.empty(a.size, np.uint8)
        if out.dtype != np.uint8 or out.size != a.size or (out.size and not out.flags.c_contiguous):
            raise ValueError("out must be a contiguous uint8 array of the input's size")
        _check(lib().hdfs_aes_ctr_xor(self.handle, stream_off, ctypes.c_void_p(a.ctypes.data if a.size else 0),
                                      ctypes.c_void_p(out.ctypes.data if out.size else 0), a.size),
               "hdfs_aes_ctr_xor")
        return out


def aes_wire_segments(pkts, prefix_off, stream_base: int = 0, src_base: int = 0, dst_base: int = 0):
    """hdfs_aes_wire_segments: the stream layout of a batch on an encrypted transfer (prefix 0, data 0,
    prefix 1, ... from stream_base) from the packets and the offsets ``frame_packets`` returns:
    (prefix stream offsets[npkts], data segments[npkts] as AES_SEGMENT_DTYPE)."""
    pkts = as_packets(pkts)
    offs = np.ascontiguousarray(prefix_off, dtype=np.uint64)
    if offs.size != pkts.size + 1:
        raise ValueError("prefix_off has npkts + 1 entries")
    segs = np.zeros(max(pkts.size, 1), AES_SEGMENT_DTYPE)
    pre = np.zeros(max(pkts.size, 1), np.uint64)
    n = int(lib().hdfs_aes_wire_segments(_np_ptr(pkts), pkts.size, _np_ptr(offs), stream_base,
                                         ctypes.c_void_p(src_base), ctypes.c_void_p(dst_base), _np_ptr(segs),
                                         _np_ptr(pre), pkts.size))
    if n < 0:
        _check(n, "hdfs_aes_wire_segments")
    return pre[:n], segs[:n]


def debug_aes_geometry() -> dict:
    """crc32c_debug_aes_geometry: the AES/CTR kernel's lane_bytes, wave_bytes, workgroup_bytes,
    list_max_segments, lanes_per_cu."""
    g = np.zeros(5, np.uint32)
    lib().crc32c_debug_aes_geometry(_np_ptr(g))
    return dict(zip(["lane_bytes", "wave_bytes", "workgroup_bytes", "list_max_segments", "lanes_per_cu"],
                    (int(x) for x in g)))


def _aes_segments(segs) -> np.ndarray:
    if not (isinstance(segs, np.ndarray) and segs.dtype == AES_SEGMENT_DTYPE):
        segs = np.array([tuple(int(v) for v in s) for s in segs], dtype=AES_SEGMENT_DTYPE)
    return np.ascontiguousarray(segs)


def debug_aes_strided_launch_info(num_cu: int, dst: int, seg_len: int, nsegs: int = 1, dst_stride: int = 0) -> dict:
    """crc32c_debug_aes_strided_launch_info: windows, wave_units, windows_per_lane and grid of the launch
    Context.aes_ctr_xor_strided would make for these arguments on num_cu CUs (no GPU)."""
    out = DebugAesLaunch()
    _check(lib().crc32c_debug_aes_strided_launch_info(num_cu, ctypes.c_void_p(dst), seg_len, nsegs, dst_stride,
                                                      ctypes.byref(out)), "crc32c_debug_aes_strided_launch_info")
    return out.as_dict()


def debug_aes_list_launch_info(num_cu: int, segs) -> dict:
    """crc32c_debug_aes_list_launch_info: the same for ONE launch of Context.aes_ctr_xor_list (at most
    AES_LIST_MAX_SEGMENTS segments, given as there)."""
    segs = _aes_segments(segs)
    out = DebugAesLaunch()
    _check(lib().crc32c_debug_aes_list_launch_info(num_cu, _np_ptr(segs) if segs.size else None, segs.size,
                                                   ctypes.byref(out)), "crc32c_debug_aes_list_launch_info")
    return out.as_dict()


# --- 8. Erasure coding (striped block groups) -------------------------------
EC_RS, EC_XOR = 0, 1  # HDFS_EC_RS, HDFS_EC_XOR
EC_MAX_DATA, EC_MAX_PARITY = 16, 4


class _EcMatrixStruct(ctypes.Structure):
    _fields_ = [("n_in", ctypes.c_uint32), ("n_out", ctypes.c_uint32), ("coef", (ctypes.c_uint8 * 16) * 4),
                ("reserved", ctypes.c_uint32 * 2)]


def gf256_mul(a: int, b: int) -> int:
    """hdfs_gf256_mul: a * b in GF(2^8) mod 0x11d."""
    return int(lib().hdfs_gf256_mul(a, b))


def gf256_inv(a: int) -> int:
    """hdfs_gf256_inv: the multiplicative inverse in GF(2^8) mod 0x11d (0 -> 0)."""
    return int(lib().hdfs_gf256_inv(a))


def _unit_ptrs(units, n: int, what: str):
    """A (void *)[n] of addresses (None / 0 = NULL) and n itself; None for no array at all."""
    if units is None:
        return None
    units = list(units)
    if len(units) != n:
        raise ValueError("%s: %d units for a matrix of %d" % (what, len(units), n))
    return (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(int(u) if u else 0) for u in units])


class EcMatrix:
    """hdfs_ec_matrix: out[r] = sum_j coef[r][j] * in[j] over GF(2^8).  ``EcMatrix.encode`` is the parity
    part of a scheme, ``EcMatrix.decode`` the recovery rows of an erasure pattern; ``apply`` is the host
    path, ``Context.ec_apply`` / ``Context.ec_encode_striped`` the device forms."""

    def __init__(self, rows=None):
        self.c = _EcMatrixStruct()
        if rows is not None:
            rows = [list(r) for r in rows]
            self.c.n_out, self.c.n_in = len(rows), len(rows[0]) if rows else 0
            for r, row in enumerate(rows[:4]):
                for j, v in enumerate(row[:16]):
                    self.c.coef[r][j] = v

    @classmethod
    def encode(cls, k: int, m: int, codec: int = EC_RS) -> "EcMatrix":
        mx = cls()
        _check(lib().hdfs_ec_encode_matrix(codec, k, m, ctypes.byref(mx.c)), "hdfs_ec_encode_matrix")
        return mx

    @classmethod
    def decode(cls, k: int, m: int, valid, erased, codec: int = EC_RS) -> "EcMatrix":
        """Column i multiplies surviving unit valid[i] (k of them), row r rebuilds unit erased[r]."""
        mx = cls()
        v = np.ascontiguousarray(valid, dtype=np.uint32)
        e = np.ascontiguousarray(erased, dtype=np.uint32)
        if v.size != k:
            raise ValueError("valid lists k = %d surviving units (%d given)" % (k, v.size))
        _check(lib().hdfs_ec_decode_matrix(codec, k, m, _np_ptr(v), _np_ptr(e) if e.size else None, e.size,
                                           ctypes.byref(mx.c)), "hdfs_ec_decode_matrix")
        return mx

    @property
    def n_in(self) -> int:
        return int(self.c.n_in)

    @property
    def n_out(self) -> int:
        return int(self.c.n_out)

    @property
    def rows(self) -> list:
        return [[int(self.c.coef[r][j]) for j in range(self.n_in)] for r in range(self.n_out)]

    @property
    def handle(self):
        return ctypes.byref(self.c)

    def apply_ptrs(self, ins, outs, length: int) -> None:
        """hdfs_ec_apply over raw host addresses (None / 0 in ``ins`` = a unit of zeros)."""
        _check(lib().hdfs_ec_apply(self.handle, _unit_ptrs(ins, self.n_in, "inputs"),
                                   _unit_ptrs(outs, self.n_out, "outputs"), length), "hdfs_ec_apply")

    def apply(self, units) -> list:
        """hdfs_ec_apply: the n_out output units of n_in input units (uint8 arrays of one length, or
        None for a unit of zeros)."""
        units = [None if u is None else np.ascontiguousarray(u, dtype=np.uint8) for u in units]
        sizes = {u.size for u in units if u is not None}
        if len(sizes) > 1:
            raise ValueError("units of different lengths")
        n = sizes.pop() if sizes else 0
        outs = [np.zeros(n, np.uint8) for _ in range(self.n_out)]
        if n:
            self.apply_ptrs([None if u is None else u.ctypes.data for u in units], [o.ctypes.data for o in outs], n)
        return outs


def ec_group_layout(length: int, k: int, m: int, cell: int) -> list:
    """hdfs_ec_group_layout: the k + m internal block lengths of a striped block group of ``length`` bytes."""
    out = np.zeros(k + m if 0 < k <= 16 and 0 < m <= 4 else 20, np.uint64)
    _check(lib().hdfs_ec_group_layout(length, k, m, cell, _np_ptr(out)), "hdfs_ec_group_layout")
    return [int(x) for x in out[:k + m]]


def ec_block_packets(length: int, k: int, cell: int, block: int, packetsize: int = 65536, bpc: int = 512,
                     out_idx0: int = 0) -> np.ndarray:
    """hdfs_ec_block_packets: the packets of data block ``block`` over the file-order buffer of a striped
    block group (payload_off steps through the block's cells at stride k * cell)."""
    n = int(lib().hdfs_ec_block_packets(length, k, cell, block, packetsize, bpc, out_idx0, None, 0))
    if n < 0:
        _check(n, "hdfs_ec_block_packets")
    pk = np.zeros(max(n, 1), PACKET_DTYPE)
    n = int(lib().hdfs_ec_block_packets(length, k, cell, block, packetsize, bpc, out_idx0, _np_ptr(pk), n))
    if n < 0:
        _check(n, "hdfs_ec_block_packets")
    return pk[:n]


def debug_ec_geometry() -> dict:
    """crc32c_debug_ec_geometry: the erasure-coding kernel's lane_bytes, wave_bytes, workgroup_bytes,
    waves_per_workgroup, table_copies, lds_bytes_per_input, lds_bytes_per_cu, max_workgroups_per_cu."""
    g = np.zeros(8, np.uint32)
    lib().crc32c_debug_ec_geometry(_np_ptr(g))
    return dict(zip(["lane_bytes", "wave_bytes", "workgroup_bytes", "waves_per_workgroup", "table_copies",
                     "lds_bytes_per_input", "lds_bytes_per_cu", "max_workgroups_per_cu"], (int(x) for x in g)))


def debug_packets_composite_shape(pkts):
    """The (bpc, last_len) crc32c_plan_create would record for the batch, or None when it is not of the
    composite shape (no GPU)."""
    pkts = as_packets(pkts)
    bpc, last = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = lib().crc32c_debug_packets_composite_shape(_np_ptr(pkts) if pkts.size else None, pkts.size,
                                                    ctypes.byref(bpc), ctypes.byref(last))
    return None if rc else (int(bpc.value), int(last.value))


def nchunks(length: int, bpc: int) -> int:
    return int(lib().crc32c_nchunks(length, bpc))


def packetize(length: int, blockoffset: int, packetsize: int, bpc: int) -> list:
    n = int(lib().crc32c_packetize(length, blockoffset, packetsize, bpc, None, 0))
    lens = np.zeros(max(n, 1), np.uint64)
    lib().crc32c_packetize(length, blockoffset, packetsize, bpc, _np_ptr(lens), n)
    return [int(x) for x in lens[:n]]


def device_count() -> int:
    return int(lib().crc32c_device_count())


# --- 2-4. GPU context, plans, host batches --------------------------------
class Context:
    """One HIP device (crc32c_ctx)."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib().crc32c_ctx_create(device, ctypes.byref(h)), "crc32c_ctx_create")
        self.handle = h
        self.device = device

    def close(self) -> None:
        if self.handle:
            lib().crc32c_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def capture_overlap(self, on: bool) -> bool:
        """crc32c_ctx_capture_overlap: whether captured Plan.exec launches that
        touch nothing in common may overlap (the default); returns the
        previous setting."""
        prev = int(lib().crc32c_ctx_capture_overlap(self.handle, 1 if on else 0))
        if prev < 0:
            _check(prev, "crc32c_ctx_capture_overlap")
        return bool(prev)

    def capture_stats(self):
        """crc32c_ctx_capture_stats: (execs captured, those with no edge from
        the previous captured exec, runs started)."""
        out = (ctypes.c_uint64 * 3)()
        _check(lib().crc32c_ctx_capture_stats(self.handle, out), "crc32c_ctx_capture_stats")
        return int(out[0]), int(out[1]), int(out[2])

    def plan(self, pkts, flags: int = 0) -> "Plan":
        return Plan(self, pkts, flags)

    def write_plan(self, buffers, bufferoffset: int, length: int, blockoffset: int = 0, packetsize: int = 65536,
                   bpc: int = 512, flags: int = 0) -> "Plan":
        """crc32c_plan_create_buffers: hadoop_rpc_send_packets over a buffer list
        [(device address or 0 for zero fill, length), ...]; exec with payload 0."""
        return Plan(self, None, flags, write=(buffers, bufferoffset, length, blockoffset, packetsize, bpc))

    def verify_frames(self, frames: np.ndarray, bpc: int, chunk_offset: int, flags: int = 0) -> FramesResult:
        """crc32c_verify_frames_host over a buffer of received packet frames."""
        return verify_frames(frames, bpc, chunk_offset, flags, ctx=self)

    def batch_host(self, payload: np.ndarray, pkts, flags: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        """Host-resident batch (crc32c_batch_host): H2D copy -> kernel -> checksums in host memory."""
        pkts = as_packets(pkts)
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        n = total_checksums(pkts)
        if out is None:
            out = np.zeros(max(n, 1), np.uint32)
        _check(lib().crc32c_batch_host(self.handle, _np_ptr(payload), _np_ptr(pkts), pkts.size, _np_ptr(out), flags),
               "crc32c_batch_host")
        return out[:n]

    def verify_host(self, payload: np.ndarray, pkts, expected: np.ndarray, flags: int = 0):
        """Host-resident verification: (number of mismatching checksums, lowest bad index or None)."""
        pkts = as_packets(pkts)
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        expected = np.ascontiguousarray(expected, dtype=np.uint32)
        first = ctypes.c_uint64(0)
        rc = lib().crc32c_verify_host(self.handle, _np_ptr(payload), _np_ptr(pkts), pkts.size, _np_ptr(expected),
                                      flags, ctypes.byref(first))
        if rc < 0:
            _check(int(rc), "crc32c_verify_host")
        return int(rc), (None if first.value == 0xFFFFFFFFFFFFFFFF else int(first.value))

    def chunks_dev(self, pkts, dev_payload: int, dev_out: int, flags: int = 0, stream: int = 0) -> None:
        pkts = as_packets(pkts)
        _check(lib().crc32c_chunks_dev(self.handle, _np_ptr(pkts), pkts.size, ctypes.c_void_p(dev_payload),
                                       ctypes.c_void_p(dev_out), flags, ctypes.c_void_p(stream)), "crc32c_chunks_dev")

    def md5_blocks(self, dev_sums: int, nsums: int, crc_per_block: int, dev_md5: int, flags: int = 0,
                   stream=0) -> None:
        """crc32c_md5_blocks: the MD5 of every crc_per_block checksums of a contiguous device array
        (the last block ragged), 16 bytes each to dev_md5; one launch, asynchronous on ``stream``.
        ``flags``: CRC32C_BIG_ENDIAN when the checksums are stored in wire order."""
        _check(lib().crc32c_md5_blocks(self.handle, ctypes.c_void_p(dev_sums), nsums, crc_per_block, flags,
                                       ctypes.c_void_p(dev_md5), ctypes.c_void_p(_stream_handle(stream, {}))),
               "crc32c_md5_blocks")

    def md5_block_list(self, dev_sums, nsums, dev_md5: int, flags: int = 0, stream=0) -> None:
        """crc32c_md5_block_list: the MD5 of nsums[i] checksums at device address dev_sums[i] (0 allowed
        where nsums[i] == 0) to dev_md5 + 16 i; one launch per MD5_LIST_MAX_BLOCKS blocks."""
        n = len(dev_sums)
        if len(nsums) != n:
            raise ValueError("dev_sums and nsums differ in length")
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(int(x)) for x in dev_sums])
        counts = (ctypes.c_uint32 * max(n, 1))(*[int(x) for x in nsums])
        _check(lib().crc32c_md5_block_list(self.handle, ptrs, counts, n, flags, ctypes.c_void_p(dev_md5),
                                           ctypes.c_void_p(_stream_handle(stream, {}))), "crc32c_md5_block_list")

    def composite_cells(self, dev_sums: int, nsums: int, crc_per_cell: int, bpc: int, last_len: int,
                        dev_crcs: int, flags: int = 0, stream=0) -> None:
        """crc32c_composite_cells: the CRC of the bytes behind every crc_per_cell checksums of a
        contiguous device array (the last cell ragged; the array's last checksum covers last_len bytes),
        one u32 each to dev_crcs; asynchronous on ``stream``.  ``flags``: CRC32C_BIG_ENDIAN (stored order
        of inputs and outputs), CRC32C_TYPE_CRC32."""
        _check(lib().crc32c_composite_cells(self.handle, ctypes.c_void_p(dev_sums), nsums, crc_per_cell, bpc,
                                            last_len, flags, ctypes.c_void_p(dev_crcs),
                                            ctypes.c_void_p(_stream_handle(stream, {}))), "crc32c_composite_cells")

    def composite_block_list(self, dev_sums, nsums, last_lens, bpc: int, dev_crcs: int, flags: int = 0,
                             stream=0) -> None:
        """crc32c_composite_block_list: the composite CRC of nsums[i] checksums at device address
        dev_sums[i] (0 allowed where nsums[i] == 0), last chunk last_lens[i] bytes, to dev_crcs[i]; one
        launch per COMPOSITE_LIST_MAX_BLOCKS blocks."""
        n = len(dev_sums)
        if len(nsums) != n or len(last_lens) != n:
            raise ValueError("dev_sums, nsums and last_lens differ in length")
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(int(x)) for x in dev_sums])
        counts = (ctypes.c_uint32 * max(n, 1))(*[int(x) for x in nsums])
        lasts = (ctypes.c_uint32 * max(n, 1))(*[int(x) for x in last_lens])
        _check(lib().crc32c_composite_block_list(self.handle, ptrs, counts, lasts, n, bpc, flags,
                                                 ctypes.c_void_p(dev_crcs),
                                                 ctypes.c_void_p(_stream_handle(stream, {}))),
               "crc32c_composite_block_list")

    def bitmap_verdicts(self, dev_bad_bits: int, nsums: int, crc_per_cell: int, dev_verdicts: int, stream=0) -> None:
        """crc32c_bitmap_verdicts: a mismatch bitmap in device memory (what Plan.verify wrote to
        dev_bad_bits) cut into cells of crc_per_cell bits -> one crc32c_block_verdict (16 bytes,
        BLOCK_VERDICT_DTYPE) per cell to dev_verdicts; one launch, asynchronous on ``stream``."""
        _check(lib().crc32c_bitmap_verdicts(self.handle, ctypes.c_void_p(dev_bad_bits), nsums, crc_per_cell,
                                            ctypes.c_void_p(dev_verdicts),
                                            ctypes.c_void_p(_stream_handle(stream, {}))), "crc32c_bitmap_verdicts")


    def aes_ctr_xor_strided(self, aes: "AesCtr", src: int, dst: int, seg_len: int, nsegs: int = 1,
                            src_stride: int = 0, dst_stride: int = 0, stream_off: int = 0, stream_stride: int = 0,
                            stream=0) -> None:
        """hdfs_aes_ctr_xor_strided_dev: segment i = seg_len bytes at src + i * src_stride, XOR-ed with
        the keystream from stream_off + i * stream_stride on, to dst + i * dst_stride (dst == src: in
        place); any alignment; ONE launch, asynchronous on ``stream``.  nsegs == 1: a contiguous range."""
        _check(lib().hdfs_aes_ctr_xor_strided_dev(self.handle, aes.handle if aes is not None else None,
                                                  ctypes.c_void_p(src), ctypes.c_void_p(dst), seg_len, nsegs,
                                                  src_stride, dst_stride, stream_off, stream_stride,
                                                  ctypes.c_void_p(_stream_handle(stream, {}))),
               "hdfs_aes_ctr_xor_strided_dev")

    def aes_ctr_xor_list(self, aes: "AesCtr", segs, stream=0) -> None:
        """hdfs_aes_ctr_xor_list_dev: ragged segments [(src, dst, stream_off, len), ...] (or an
        AES_SEGMENT_DTYPE array; addresses 0 allowed where len == 0); one launch per
        AES_LIST_MAX_SEGMENTS segments, asynchronous on ``stream``."""
        segs = _aes_segments(segs)
        _check(lib().hdfs_aes_ctr_xor_list_dev(self.handle, aes.handle if aes is not None else None,
                                               _np_ptr(segs) if segs.size else None, segs.size,
                                               ctypes.c_void_p(_stream_handle(stream, {}))),
               "hdfs_aes_ctr_xor_list_dev")


    def ec_apply(self, mx: "EcMatrix", dev_in, dev_out, length: int, stream=0) -> None:
        """hdfs_ec_apply_dev: out[r][t] = sum_j coef[r][j] * in[j][t] for t < length over device units
        (addresses; None / 0 in ``dev_in`` = zeros); any alignment; ONE launch, asynchronous on ``stream``."""
        n_in, n_out = (mx.n_in, mx.n_out) if mx is not None else (len(dev_in or ()), len(dev_out or ()))
        _check(lib().hdfs_ec_apply_dev(self.handle, mx.handle if mx is not None else None,
                                       _unit_ptrs(dev_in, n_in, "inputs"), _unit_ptrs(dev_out, n_out, "outputs"),
                                       length, ctypes.c_void_p(_stream_handle(stream, {}))), "hdfs_ec_apply_dev")

    def ec_encode_striped(self, mx: "EcMatrix", src: int, length: int, cell: int, dev_parity, stream=0) -> None:
        """hdfs_ec_encode_striped_dev: every stripe of a block group of ``length`` bytes at ``src`` in file
        order; parity row r of stripe s goes to dev_parity[r] + s * cell; ONE launch."""
        n_out = mx.n_out if mx is not None else len(dev_parity or ())
        _check(lib().hdfs_ec_encode_striped_dev(self.handle, mx.handle if mx is not None else None,
                                                ctypes.c_void_p(src), length, cell,
                                                _unit_ptrs(dev_parity, n_out, "parity units"),
                                                ctypes.c_void_p(_stream_handle(stream, {}))),
               "hdfs_ec_encode_striped_dev")


class Plan:
    """Device-resident batch plan (crc32c_plan): build once, execute many.

    ``stream`` is a raw HIP stream handle or an object with a ``cuda_stream`` attribute (a
    ``torch.cuda.Stream``). The C library touches every stream a plan ran on when the plan is
    destroyed (include/hdfs_crc32c.h, crc32c_plan_destroy), so a plan must be destroyed before
    its launch streams; a stream object passed here is kept alive by the plan until ``close()``.
    """

    def __init__(self, ctx: Context, pkts, flags: int = 0, write=None):
        h = ctypes.c_void_p()
        if write is None:
            pkts = as_packets(pkts)
            _check(lib().crc32c_plan_create(ctx.handle, _np_ptr(pkts), pkts.size, flags, ctypes.byref(h)),
                   "crc32c_plan_create")
        else:
            buffers, bufferoffset, length, blockoffset, packetsize, bpc = write
            bufs = as_buffers(buffers)
            _check(lib().crc32c_plan_create_buffers(ctx.handle, _np_ptr(bufs), bufs.size, bufferoffset, length,
                                                    blockoffset, packetsize, bpc, flags, ctypes.byref(h)),
                   "crc32c_plan_create_buffers")
        self.ctx = ctx  # keeps the context alive
        self.handle = h
        self._streams = {}  # stream objects launched on, kept alive until close()
        self.nchecksums = int(lib().crc32c_plan_nchecksums(h))
        self.payload_bytes = int(lib().crc32c_plan_payload_bytes(h))

    def _stream(self, stream) -> int:
        return _stream_handle(stream, self._streams)

    def exec(self, dev_payload: int, dev_out: int, stream=0) -> None:
        stream = self._stream(stream)
        _check(lib().crc32c_plan_exec(self.handle, ctypes.c_void_p(dev_payload), ctypes.c_void_p(dev_out),
                                      ctypes.c_void_p(stream)), "crc32c_plan_exec")

    def verify(self, dev_payload: int, dev_expected: int, dev_result: int, stream=0,
               dev_bad_bits: int = 0) -> None:
        """Compare instead of store: dev_result[0] = mismatches, [1] = lowest bad index (async); with
        dev_bad_bits (ceil(nchecksums / 32) u32s) also the bitmap of mismatching checksums
        (crc32c_plan_verify_bitmap)."""
        stream = self._stream(stream)
        if dev_bad_bits:
            _check(lib().crc32c_plan_verify_bitmap(self.handle, ctypes.c_void_p(dev_payload),
                                                   ctypes.c_void_p(dev_expected), ctypes.c_void_p(dev_result),
                                                   ctypes.c_void_p(dev_bad_bits), ctypes.c_void_p(stream)),
                   "crc32c_plan_verify_bitmap")
            return
        _check(lib().crc32c_plan_verify(self.handle, ctypes.c_void_p(dev_payload), ctypes.c_void_p(dev_expected),
                                        ctypes.c_void_p(dev_result), ctypes.c_void_p(stream)), "crc32c_plan_verify")

    def exec_blocks(self, dev_payloads, dev_outs, stream=0) -> None:
        """crc32c_plan_exec_blocks: this plan (one block's shape) on every block, one launch per <= 32."""
        stream = self._stream(stream)
        n = len(dev_payloads)
        pays = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_payloads])
        outs = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_outs])
        _check(lib().crc32c_plan_exec_blocks(self.handle, pays, outs, n, ctypes.c_void_p(stream)),
               "crc32c_plan_exec_blocks")

    def verify_blocks_work_bytes(self, nblocks: int) -> int:
        """crc32c_plan_verify_blocks_work_bytes: the bytes of device scratch verify_blocks needs for nblocks
        blocks (the bitmap over nblocks * nchecksums checksums, then two u32 per launch of 32 blocks)."""
        return int(lib().crc32c_plan_verify_blocks_work_bytes(self.handle, nblocks))

    def verify_blocks(self, dev_payloads, dev_expected: int, dev_verdicts: int, dev_work: int, stream=0) -> None:
        """crc32c_plan_verify_blocks: this plan (one block's shape) compared on every block -- block b's
        payload at dev_payloads[b], its expected checksums at dev_expected + 4 * b * nchecksums -- one
        verify launch per 32 blocks and one verdict launch: a crc32c_block_verdict (BLOCK_VERDICT_DTYPE)
        per block to dev_verdicts, the mismatch bitmap of all blocks at the start of dev_work."""
        stream = self._stream(stream)
        n = len(dev_payloads)
        pays = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_payloads])
        _check(lib().crc32c_plan_verify_blocks(self.handle, pays, ctypes.c_void_p(dev_expected), n,
                                               ctypes.c_void_p(dev_verdicts), ctypes.c_void_p(dev_work),
                                               ctypes.c_void_p(stream)), "crc32c_plan_verify_blocks")

    def exec_blocks_md5(self, dev_payloads, dev_outs, dev_md5: int, stream=0) -> None:
        """crc32c_plan_exec_blocks_md5: exec_blocks, then each block's MD5 (16 bytes to dev_md5 + 16 i)
        on the same stream; the checksums' stored order is the plan's."""
        stream = self._stream(stream)
        n = len(dev_payloads)
        pays = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_payloads])
        outs = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_outs])
        _check(lib().crc32c_plan_exec_blocks_md5(self.handle, pays, outs, n, ctypes.c_void_p(dev_md5),
                                                 ctypes.c_void_p(stream)), "crc32c_plan_exec_blocks_md5")

    def exec_blocks_composite(self, dev_payloads, dev_outs, dev_crcs: int, stream=0) -> None:
        """crc32c_plan_exec_blocks_composite: exec_blocks, then each block's composite CRC (one u32 to
        dev_crcs[i], stored in the plan's order) on the same stream; the plan must have the composite
        shape (composite_shape)."""
        stream = self._stream(stream)
        n = len(dev_payloads)
        pays = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_payloads])
        outs = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_outs])
        _check(lib().crc32c_plan_exec_blocks_composite(self.handle, pays, outs, n, ctypes.c_void_p(dev_crcs),
                                                       ctypes.c_void_p(stream)), "crc32c_plan_exec_blocks_composite")

    def composite_shape(self):
        """crc32c_plan_composite_shape: (bpc, last_len) when the plan's checksums combine into the CRC of
        its bytes with these two lengths; Crc32cError(-EINVAL) otherwise."""
        bpc, last = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().crc32c_plan_composite_shape(self.handle, ctypes.byref(bpc), ctypes.byref(last)),
               "crc32c_plan_composite_shape")
        return int(bpc.value), int(last.value)

    def blocks(self, max_blocks: int = 16, window_us: int = 20, resident: bool = False,
               idle_us: int = 0) -> "Blocks":
        """The block queue (crc32c_blocks_create), or its resident-kernel mode
        (crc32c_blocks_create_resident) with ``resident=True``."""
        return Blocks(self, max_blocks, window_us, resident=resident, idle_us=idle_us)

    def exec_variant(self, dev_payload: int, dev_out: int, variant: int, dev_stamps: int = 0, stream: int = 0) -> None:
        """Diagnostic (debug library): run an explicit kernel variant (5/6/36 write per-wave timestamps)."""
        _check(debug_lib().crc32c_debug_plan_exec_variant(self.handle, ctypes.c_void_p(dev_payload),
                                                          ctypes.c_void_p(dev_out), ctypes.c_void_p(dev_stamps),
                                                          variant, ctypes.c_void_p(stream)),
               "crc32c_debug_plan_exec_variant")

    def launch_info(self, dev_payload: int = 0, verify: bool = False) -> DebugLaunchInfo:
        """crc32c_debug_plan_launch_info: what exec (or verify) on dev_payload would launch; launches nothing."""
        info = DebugLaunchInfo()
        _check(lib().crc32c_debug_plan_launch_info(self.handle, ctypes.c_void_p(dev_payload), int(verify),
                                                   ctypes.byref(info)), "crc32c_debug_plan_launch_info")
        return info

    def blocks_launch_info(self, dev_payloads, dev_outs=None, verify: bool = False) -> list:
        """crc32c_debug_plan_blocks_launch_info: a DebugBlocksLaunch for every launch exec_blocks (verify:
        the verify launches of verify_blocks) would make over these blocks; launches nothing."""
        n = len(dev_payloads)
        pays = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_payloads])
        outs = None
        if dev_outs is not None:
            assert len(dev_outs) == n
            outs = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(x) for x in dev_outs])
        info = (DebugBlocksLaunch * max(n, 1))()  # (never more launches than blocks)
        rc = lib().crc32c_debug_plan_blocks_launch_info(self.handle, pays, outs, n, int(verify), info, max(n, 1))
        if rc < 0:
            _check(rc, "crc32c_debug_plan_blocks_launch_info")
        return list(info[:rc])

    def close(self) -> None:
        if self.handle:
            lib().crc32c_plan_destroy(self.handle)
            self.handle = None
        self._streams = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Blocks:
    """crc32c_blocks: block writes from several threads coalesced into one launch (group commit)."""

    def __init__(self, plan: Plan, max_blocks: int = 16, window_us: int = 20, resident: bool = False,
                 idle_us: int = 0):
        h = ctypes.c_void_p()
        if resident:
            _check(lib().crc32c_blocks_create_resident(plan.handle, idle_us, ctypes.byref(h)),
                   "crc32c_blocks_create_resident")
        else:
            _check(lib().crc32c_blocks_create(plan.handle, max_blocks, window_us, ctypes.byref(h)),
                   "crc32c_blocks_create")
        self.plan = plan  # the plan outlives the queue
        self.handle = h

    def submit(self, dev_payload: int, dev_out: int, plan: "Plan | None" = None) -> int:
        """crc32c_block_submit (plan None: the queue's) / crc32c_block_submit_plan
        (a block of another shape; the plan must outlive its blocks' waits)."""
        t = ctypes.c_uint64(0)
        _check(lib().crc32c_block_submit_plan(self.handle, None if plan is None else plan.handle,
                                              ctypes.c_void_p(dev_payload), ctypes.c_void_p(dev_out),
                                              ctypes.byref(t)), "crc32c_block_submit_plan")
        return int(t.value)

    def flush(self) -> None:
        _check(lib().crc32c_block_flush(self.handle), "crc32c_block_flush")

    def wait(self, ticket: int) -> None:
        _check(lib().crc32c_block_wait(self.handle, ticket), "crc32c_block_wait")

    def checksums(self, dev_payload: int, dev_out: int) -> None:
        """Submit + wait: returns when the block's checksums are in dev_out."""
        _check(lib().crc32c_block_checksums(self.handle, ctypes.c_void_p(dev_payload), ctypes.c_void_p(dev_out)),
               "crc32c_block_checksums")

    def debug_fail_flushes(self, n: int) -> None:
        """crc32c_debug_blocks_fail_flushes: the next n flushes fail at issue (tests of the error path)."""
        _check(lib().crc32c_debug_blocks_fail_flushes(self.handle, n), "crc32c_debug_blocks_fail_flushes")

    def debug_resident_inject(self, hold: bool, fail_waits: int = 0) -> None:
        """crc32c_debug_blocks_resident_inject: hold = no kernel launch (submits queue
        up); the next fail_waits waits return -ETIMEDOUT at once."""
        _check(lib().crc32c_debug_blocks_resident_inject(self.handle, int(hold), fail_waits),
               "crc32c_debug_blocks_resident_inject")

    def stats(self):
        f, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().crc32c_blocks_stats(self.handle, ctypes.byref(f), ctypes.byref(b)), "crc32c_blocks_stats")
        return int(f.value), int(b.value)

    def close(self) -> None:
        if self.handle:
            lib().crc32c_blocks_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_unique_id() -> bytes:
    """crc32c_multi_unique_id: the 128-byte RCCL id rank 0 sends to the other ranks."""
    buf = (ctypes.c_uint8 * 128)()
    _check(lib().crc32c_multi_unique_id(buf), "crc32c_multi_unique_id")
    return bytes(buf)


class Multi:
    """Several GPUs of one node (crc32c_multi): all devices of this process
    (``Multi([0, 1, ...])``), or one device of a one-process-per-GPU job
    (``Multi(device=d, rank=r, nranks=n, uid=bytes)``)."""

    def __init__(self, devices=None, device: int = 0, rank: int = 0, nranks: int = 1, uid: bytes | None = None):
        h = ctypes.c_void_p()
        if uid is None:
            devs = (ctypes.c_int * len(devices))(*devices)
            _check(lib().crc32c_multi_create(devs, len(devices), ctypes.byref(h)), "crc32c_multi_create")
            self.local_devices = list(devices)
        else:
            idb = (ctypes.c_uint8 * 128)(*uid)
            _check(lib().crc32c_multi_create_rank(device, rank, nranks, idb, ctypes.byref(h)),
                   "crc32c_multi_create_rank")
            self.local_devices = [device]
        self.handle = h

    def plan(self, pkts, group_packets: int = 64, flags: int = 0) -> "MultiPlan":
        return MultiPlan(self, pkts, group_packets, flags)

    def capture_stats(self, local: int = 0):
        """Context.capture_stats of local device ``local``'s context."""
        out = (ctypes.c_uint64 * 3)()
        _check(lib().crc32c_debug_multi_capture_stats(self.handle, local, out), "crc32c_debug_multi_capture_stats")
        return int(out[0]), int(out[1]), int(out[2])

    def sync(self) -> None:
        _check(lib().crc32c_multi_sync(self.handle), "crc32c_multi_sync")

    def batch_host(self, payload: np.ndarray, pkts, group_packets: int = 64, flags: int = 0) -> np.ndarray:
        pkts = as_packets(pkts)
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        n = total_checksums(pkts)
        out = np.zeros(max(n, 1), np.uint32)
        _check(lib().crc32c_multi_batch_host(self.handle, _np_ptr(payload), _np_ptr(pkts), pkts.size, group_packets,
                                             _np_ptr(out), flags), "crc32c_multi_batch_host")
        return out[:n]

    def close(self) -> None:
        if self.handle:
            lib().crc32c_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiPlan:
    """Device-resident multi-GPU plan (crc32c_multi_plan): shards + RCCL gather to rank 0."""

    def __init__(self, multi: Multi, pkts, group_packets: int = 64, flags: int = 0):
        pkts = as_packets(pkts)
        h = ctypes.c_void_p()
        _check(lib().crc32c_multi_plan_create(multi.handle, _np_ptr(pkts), pkts.size, group_packets, flags,
                                              ctypes.byref(h)), "crc32c_multi_plan_create")
        self.multi = multi
        self.handle = h
        self._streams = {}  # stream objects launched on, kept alive until close()
        self.nchecksums = int(lib().crc32c_multi_plan_nchecksums(h))

    def shard_bytes(self, rank: int) -> int:
        return int(lib().crc32c_multi_plan_shard_bytes(self.handle, rank))

    def gather_ops(self):
        """crc32c_multi_plan_gather_ops: (point-to-point operations one exec
        posts over the communicator, packed: staging array + scatter kernel)."""
        packed = ctypes.c_int(0)
        n = int(lib().crc32c_multi_plan_gather_ops(self.handle, ctypes.byref(packed)))
        return n, bool(packed.value)

    def exec(self, dev_shards, root_out: int, streams=None) -> None:
        """``streams``: one per local device, handles or stream objects (kept
        alive until close(): the next exec on another stream records an event
        on this one)."""
        n = len(dev_shards)
        shards = (ctypes.c_void_p * n)(*[ctypes.c_void_p(x) for x in dev_shards])
        ss = None if streams is None else (ctypes.c_void_p * n)(
            *[ctypes.c_void_p(_stream_handle(x, self._streams)) for x in streams])
        _check(lib().crc32c_multi_plan_exec(self.handle, shards, ctypes.c_void_p(root_out), ss),
               "crc32c_multi_plan_exec")

    def join(self, streams=None) -> None:
        """crc32c_multi_plan_join (CRC32C_MULTI_PIPELINE plans): every local
        stream waits for every exec issued so far."""
        n = len(self.multi.local_devices)
        ss = None if streams is None else (ctypes.c_void_p * n)(
            *[ctypes.c_void_p(_stream_handle(x, self._streams)) for x in streams])
        _check(lib().crc32c_multi_plan_join(self.handle, ss), "crc32c_multi_plan_join")

    def close(self) -> None:
        if self.handle:
            lib().crc32c_multi_plan_destroy(self.handle)
            self.handle = None
        self._streams = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_layout(pkts, group_packets: int, nranks: int):
    """crc32c_multi_layout: (per-group [rank, shard offset, payload offset, bytes] rows, shard bytes per rank)."""
    pkts = as_packets(pkts)
    n = int(lib().crc32c_multi_layout(_np_ptr(pkts), pkts.size, group_packets, nranks, None, None))
    if n < 0:
        _check(n, "crc32c_multi_layout")
    lay = np.zeros((max(n, 1), 4), np.uint64)
    sb = np.zeros(nranks, np.uint64)
    lib().crc32c_multi_layout(_np_ptr(pkts), pkts.size, group_packets, nranks, _np_ptr(lay), _np_ptr(sb))
    return lay[:n], sb


def multi_shard_packets(pkts, group_packets: int, nranks: int, rank: int) -> np.ndarray:
    """crc32c_multi_shard_packets: rank's packets, payload offsets into its shard, global out indices."""
    pkts = as_packets(pkts)
    n = int(lib().crc32c_multi_shard_packets(_np_ptr(pkts), pkts.size, group_packets, nranks, rank, None, 0))
    if n < 0:
        _check(n, "crc32c_multi_shard_packets")
    out = np.zeros(max(n, 1), PACKET_DTYPE)
    lib().crc32c_multi_shard_packets(_np_ptr(pkts), pkts.size, group_packets, nranks, rank, _np_ptr(out), n)
    return out[:n]


def multi_rank_packets(pkts, group_packets: int, nranks: int, rank: int, flags: int = 0) -> np.ndarray:
    """crc32c_multi_rank_packets: the packets rank's plan computes (payload offsets into its shard, out
    indices into the array it sends to rank 0; rank 0's global unless CRC32C_MULTI_SELF_SEND)."""
    pkts = as_packets(pkts)
    n = int(lib().crc32c_multi_rank_packets(_np_ptr(pkts), pkts.size, group_packets, nranks, rank, flags, None, 0))
    if n < 0:
        _check(n, "crc32c_multi_rank_packets")
    out = np.zeros(max(n, 1), PACKET_DTYPE)
    lib().crc32c_multi_rank_packets(_np_ptr(pkts), pkts.size, group_packets, nranks, rank, flags, _np_ptr(out), n)
    return out[:n]


def multi_transfers(pkts, group_packets: int, nranks: int, flags: int = 0):
    """crc32c_multi_transfers: (local_nout[nranks], transfers[T, 4] = {sending rank, index in its local array,
    file index on rank 0, count}) -- the exchange crc32c_multi_plan_exec posts, in posting order."""
    pkts = as_packets(pkts)
    n = int(lib().crc32c_multi_transfers(_np_ptr(pkts), pkts.size, group_packets, nranks, flags, None, None, 0))
    if n < 0:
        _check(n, "crc32c_multi_transfers")
    ln = np.zeros(nranks, np.uint64)
    xs = np.zeros((max(n, 1), 4), np.uint64)
    lib().crc32c_multi_transfers(_np_ptr(pkts), pkts.size, group_packets, nranks, flags, _np_ptr(ln), _np_ptr(xs), n)
    return ln, xs[:n]


def multi_scatter(pkts, group_packets: int, nranks: int, flags: int = 0):
    """crc32c_multi_scatter: the packed gather's layout -- (stage_off[nranks], tiles[T, 3] = {staging index,
    file index, count}); T = 0 when the gather is not packed (one send / receive per placement)."""
    pkts = as_packets(pkts)
    n = int(lib().crc32c_multi_scatter(_np_ptr(pkts), pkts.size, group_packets, nranks, flags, None, None, 0))
    if n < 0:
        _check(n, "crc32c_multi_scatter")
    so = np.zeros(nranks, np.uint64)
    ts = np.zeros((max(n, 1), 3), np.uint64)
    lib().crc32c_multi_scatter(_np_ptr(pkts), pkts.size, group_packets, nranks, flags, _np_ptr(so), _np_ptr(ts), n)
    return so, ts[:n]


def verify_frames(frames: np.ndarray, bpc: int, chunk_offset: int, flags: int = 0, ctx: Context | None = None):
    """crc32c_verify_frames_host over a buffer of received packet frames; ctx None (no GPU) needs
    CRC32C_CPU_FALLBACK."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    res = FramesResult()
    _check(lib().crc32c_verify_frames_host(None if ctx is None else ctx.handle, _np_ptr(frames), frames.size, bpc,
                                           chunk_offset, flags, ctypes.byref(res)), "crc32c_verify_frames_host")
    return res


def parse_frames(frames: np.ndarray):
    """crc32c_parse_frames: (frame records, bytes consumed)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    used = ctypes.c_uint64(0)
    n = int(lib().crc32c_parse_frames(_np_ptr(frames), frames.size, None, 0, ctypes.byref(used)))
    if n < 0:
        _check(n, "crc32c_parse_frames")
    info = np.zeros(max(n, 1), FRAME_DTYPE)
    lib().crc32c_parse_frames(_np_ptr(frames), frames.size, _np_ptr(info), n, ctypes.byref(used))
    return info[:n], int(used.value)


def last_path() -> int:
    return int(lib().crc32c_last_path())


def as_buffers(buffers) -> np.ndarray:
    if isinstance(buffers, np.ndarray) and buffers.dtype == BUFFER_DTYPE:
        return np.ascontiguousarray(buffers)
    return np.array([(int(d or 0), int(n)) for d, n in buffers], BUFFER_DTYPE)


def debug_write_plan(buffers, bufferoffset: int, length: int, blockoffset: int = 0, packetsize: int = 65536,
                     bpc: int = 512) -> dict:
    bufs = as_buffers(buffers)
    c = np.zeros(6, np.uint64)
    _check(lib().crc32c_debug_write_plan(_np_ptr(bufs), bufs.size, bufferoffset, length, blockoffset, packetsize,
                                         bpc, _np_ptr(c)), "crc32c_debug_write_plan")
    return dict(zip(["tiles", "gen", "seg", "pieces", "consts", "nchecksums"], (int(x) for x in c)))


def chunks_cpu(packet: np.ndarray, bpc: int, flags: int = 0) -> np.ndarray:
    """The reference's per-packet loop on one host packet, on the host CPU."""
    packet = np.ascontiguousarray(packet, dtype=np.uint8)
    n = nchunks(packet.size, bpc)
    out = np.zeros(max(n, 1), np.uint32)
    _check(lib().crc32c_chunks_cpu(_np_ptr(packet), packet.size, bpc, _np_ptr(out), flags), "crc32c_chunks_cpu")
    return out[:n]


def batch_host_cpu(payload: np.ndarray, pkts, flags: int = 0, out: np.ndarray | None = None) -> np.ndarray:
    """The product's host-CPU path over a host batch (crc32c_batch_host with no GPU context and
    CRC32C_CPU_FALLBACK: crc32c_chunks_cpu per packet on the calling thread)."""
    pkts = as_packets(pkts)
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    n = total_checksums(pkts)
    if out is None:
        out = np.zeros(max(n, 1), np.uint32)
    _check(lib().crc32c_batch_host(None, _np_ptr(payload), _np_ptr(pkts), pkts.size, _np_ptr(out),
                                   flags | CRC32C_CPU_FALLBACK), "crc32c_batch_host (CPU)")
    return out[:n]


def chunks(packet: np.ndarray, bpc: int, flags: int = 0) -> np.ndarray:
    """The reference's per-packet loop on one host packet, on the default GPU context."""
    packet = np.ascontiguousarray(packet, dtype=np.uint8)
    n = nchunks(packet.size, bpc)
    out = np.zeros(max(n, 1), np.uint32)
    _check(lib().crc32c_chunks(_np_ptr(packet), packet.size, bpc, _np_ptr(out), flags), "crc32c_chunks")
    return out[:n]


# --- helpers ----------------------------------------------------------------
def total_checksums(pkts) -> int:
    pkts = as_packets(pkts)
    return int(lib().crc32c_batch_nchecksums(_np_ptr(pkts), pkts.size))


def debug_plan(pkts, absolute: bool = False):
    """Work items a plan would upload (FastTile / GenItem arrays); absolute:
    of a CRC32C_DEVICE_ADDRESSES plan, before it is rebased."""
    pkts = as_packets(pkts)
    nt, ng = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().crc32c_debug_plan_abs(_np_ptr(pkts), pkts.size, int(absolute), None, 0, None, 0, ctypes.byref(nt),
                                       ctypes.byref(ng)), "crc32c_debug_plan")
    tiles = np.zeros(max(nt.value, 1), TILE_DTYPE)
    gen = np.zeros(max(ng.value, 1), GEN_DTYPE)
    _check(lib().crc32c_debug_plan_abs(_np_ptr(pkts), pkts.size, int(absolute), _np_ptr(tiles), nt.value,
                                       _np_ptr(gen), ng.value, ctypes.byref(nt), ctypes.byref(ng)),
           "crc32c_debug_plan")
    return tiles[: nt.value], gen[: ng.value]


def debug_select_build(ntiles: int, ngen: int, nseg: int, nconst: int, general: int, verify: bool,
                       num_cu: int) -> DebugBuild:
    """crc32c_debug_select_build: the production build the launch path chooses (no GPU)."""
    b = DebugBuild()
    _check(lib().crc32c_debug_select_build(ntiles, ngen, nseg, nconst, general, int(verify), num_cu, ctypes.byref(b)),
           "crc32c_debug_select_build")
    return b


def debug_packets_flags(pkts, absolute: bool = False):
    """crc32c_debug_packets_flags: (KParams general bits, needs_z) of a packet batch's plan (no GPU)."""
    pkts = as_packets(pkts)
    g, z = ctypes.c_uint32(0), ctypes.c_int(0)
    _check(lib().crc32c_debug_packets_flags(_np_ptr(pkts), pkts.size, int(absolute), ctypes.byref(g), ctypes.byref(z)),
           "crc32c_debug_packets_flags")
    return int(g.value), bool(z.value)


def debug_lds_image():
    """The kernel's LDS image and affine constants (c_lg[5], c_small[4])."""
    n = int(lib().crc32c_debug_lds_image(None, 0, None, None))
    img = np.zeros(n, np.uint8)
    c_lg = np.zeros(5, np.uint32)
    c_small = np.zeros(4, np.uint32)
    lib().crc32c_debug_lds_image(_np_ptr(img), n, _np_ptr(c_lg), _np_ptr(c_small))
    return img, c_lg, c_small


def debug_lds_image_s4(flags: int = 0):
    """The slicing-by-4 kernel's LDS image (CRC32C, or CRC32 with CRC32C_TYPE_CRC32)."""
    n = int(lib().crc32c_debug_lds_image_s4(None, 0, flags))
    img = np.zeros(n, np.uint8)
    lib().crc32c_debug_lds_image_s4(_np_ptr(img), n, flags)
    return img


def debug_lds_image_s4_split(flags: int = 0):
    """The split S4 image the large-batch builds stage (16 columns per byte table)."""
    n = int(lib().crc32c_debug_lds_image_s4_split(None, 0, flags))
    img = np.zeros(n, np.uint8)
    lib().crc32c_debug_lds_image_s4_split(_np_ptr(img), n, flags)
    return img


def debug_affine_constants(flags: int = 0):
    c_lg = np.zeros(5, np.uint32)
    c_small = np.zeros(4, np.uint32)
    lib().crc32c_debug_affine_constants(flags, _np_ptr(c_lg), _np_ptr(c_small))
    return c_lg, c_small
