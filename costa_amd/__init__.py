"""costa_amd — Python view of the MI355X-native COSTA tile path.

A thin ctypes layer over ``costa_amd/lib/libcosta_amd.so`` (C ABI: include/costa_hip.h).
Names, argument meaning and error behaviour follow the reference's C++ API so tests read
like the reference's own:

    block_cyclic_layout(...)      eth-cscs/COSTA src/costa/layout.hpp:70-86
    custom_layout(...)            src/costa/layout.hpp:34-42
    transform(A, C, comm, ...)    src/costa/grid2grid/transform.hpp:13-43
    transformer(comm)             src/costa/grid2grid/transformer.hpp:8-62
    copy_and_transform(...)       src/costa/grid2grid/memory_utils.hpp:339-412

All compute runs in the HIP library; there is no Python or CPU fallback: a missing or
unloadable library raises ``CostaError`` on first use.

Pointers are plain integers (``tensor.data_ptr()``, ``ndarray.ctypes.data``); they may be
device memory (used in place) or host memory (staged through HBM by the library).
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from dataclasses import dataclass
from typing import Iterable, Sequence

import numpy as np

__all__ = [
    "CostaError", "lib", "FLOAT", "DOUBLE", "CFLOAT", "CDOUBLE", "INT32", "HALF", "BFLOAT16",
    "FP8_E4M3", "FP8_E5M2", "FP4_E2M1", "FP6_E2M3", "FP6_E3M2", "dtype_code", "element_code",
    "np_dtype", "Layout", "block_cyclic_layout", "custom_layout", "Comm", "transform",
    "transform_batch", "transform_async", "transform_batch_async", "synchronize", "transformer", "copy_and_transform", "execute_tiles", "execute_tiles_mixed",
    "convert_subtile", "TileOp", "TriOp", "TRI_OP_DTYPE", "transform_tri", "transform_tri_async",
    "execute_tiles_tri", "plan_export_tri", "tri_cut", "tri_subtile", "tri_phase_ms",
    "plan_export", "set_profiling", "get_stats", "release_caches", "TILE_OP_DTYPE",
    "ScaledOp", "SCALED_OP_DTYPE", "SCALED_F_ROWS", "transform_scaled", "execute_tiles_scaled",
    "plan_export_scaled", "scaled_subtile", "scaled_items", "mx_subtile", "block_subtile",
    "transform_amax", "layout_amax", "execute_tiles_amax", "amax_items",
    "MxScales", "MX_ROWS", "MX_COLS", "MX_FLOOR", "MX_CEIL", "mx_scales", "transform_mx",
    "execute_tiles_mx", "mx_items", "sr_bits", "mx_check_ops", "mx_check_scales",
    "BlockScales", "BLOCK_EXACT", "BLOCK_POW2", "block_scales", "transform_block_scaled",
    "execute_tiles_block_scaled", "block_items", "block_check_ops", "block_check_scales",
]

FLOAT, DOUBLE, CFLOAT, CDOUBLE, INT32 = 0, 1, 2, 3, 4
# 2-byte element types (costa_hip.h, "Half precision"): IEEE binary16 and bfloat16, raw bits.  The
# pairs are H -> H, FLOAT -> H and H -> FLOAT on device-resident layouts, and alpha / beta are fp32.
HALF, BFLOAT16 = 5, 6
_NP = {FLOAT: np.float32, DOUBLE: np.float64, CFLOAT: np.complex64,
       CDOUBLE: np.complex128, INT32: np.int32, HALF: np.float16, BFLOAT16: np.uint16}
# torch dtype objects by name (recognised without importing torch)
_TORCH = {"torch.float32": FLOAT, "torch.float64": DOUBLE, "torch.complex64": CFLOAT,
          "torch.complex128": CDOUBLE, "torch.int32": INT32, "torch.float16": HALF,
          "torch.bfloat16": BFLOAT16}

# 1-byte element types (costa_hip.h, "FP8"): OCP e4m3fn and e5m2, raw bits (np.uint8).  The pairs
# are Q -> Q, FLOAT -> Q and Q -> FLOAT on device-resident layouts, and alpha / beta are fp32.  They
# are kept out of _NP and _TORCH: dtype_code() does not know them, element_code() does.
FP8_E4M3, FP8_E5M2 = 7, 8
_NP_FP8 = {FP8_E4M3: np.uint8, FP8_E5M2: np.uint8}
_TORCH_FP8 = {"torch.float8_e4m3fn": FP8_E4M3, "torch.float8_e5m2": FP8_E5M2}
# The packed 4-bit type (costa_hip.h, "MXFP4"): OCP e2m1, two codes per byte (np.uint8 holds a PAIR:
# the even element in bits 3..0), every layout count in elements.  Only transform_mx,
# execute_tiles_mx and plan_export_scaled take it; alpha / beta are fp32.
FP4_E2M1 = 9
_NP_FP8[FP4_E2M1] = np.uint8
_TORCH_FP8["torch.float4_e2m1fn_x2"] = FP4_E2M1
# The packed 6-bit types (costa_hip.h, "MXFP6"): OCP e2m3 / e3m2, four codes per three bytes (np.uint8
# is the storage: 3 bytes hold 4 elements, the first in the lowest bits), every layout count in
# elements.  torch has no FP6 dtype: pass the code over uint8 storage.  Only transform_mx,
# execute_tiles_mx and plan_export_scaled take them; alpha / beta are fp32.
FP6_E2M3, FP6_E3M2 = 10, 11
_NP_FP8[FP6_E2M3] = np.uint8
_NP_FP8[FP6_E3M2] = np.uint8
_FP32_SCALARS = (HALF, BFLOAT16, FP8_E4M3, FP8_E5M2, FP4_E2M1, FP6_E2M3, FP6_E3M2)

TILE_TRANSPOSE, TILE_CONJ, TILE_VEC_SRC, TILE_VEC_DST = 0x1, 0x2, 0x4, 0x8
SCALE_BITCOPY, SCALE_ZERO, SCALE_ALPHA, SCALE_AXPBY = 0, 1, 2, 3

# numpy view of costa_tile_op_t (40 bytes)
TILE_OP_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("nf", "<i4"), ("ns", "<i4"),
                          ("lds", "<i4"), ("ldd", "<i4"), ("flags", "<u4"),
                          ("order", "<u4")])


# numpy view of costa_tri_op_t (48 bytes): the tile op's fields, then the diagonal
TRI_LE = 0x40
TRI_OP_DTYPE = np.dtype(TILE_OP_DTYPE.descr + [("diag", "<i4"), ("pad", "<i4")])


# numpy view of costa_scaled_op_t (48 bytes): the tile op, then the target coordinates of its source
# element (0, 0); flag SCALED_F_ROWS: the op's fast index walks target rows
SCALED_F_ROWS = 0x80
SCALED_OP_DTYPE = np.dtype([("op", TILE_OP_DTYPE), ("row0", "<i4"), ("col0", "<i4")])

# numpy view of costa_dual_op_t (64 bytes): the scaled op of output 1, then output 2's address, leading
# dimension and store mode (TILE_TRANSPOSE: dst2(f*ldd2 + s), else dst2(s*ldd2 + f))
DUAL_OP_DTYPE = np.dtype([("s", SCALED_OP_DTYPE), ("dst2", "<u8"), ("ldd2", "<i4"), ("flags2", "<u4")])


class CostaError(RuntimeError):
    """Raised when the native library reports an error (status != COSTA_OK)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[costa status {code}] {msg}")
        self.code = code


def dtype_code(dtype) -> int:
    """The element-type code of a code, a numpy dtype (``np.float16`` is HALF; numpy has no
    bfloat16) or a torch dtype object (``torch.bfloat16`` is BFLOAT16)."""
    if isinstance(dtype, int):
        return dtype
    if type(dtype).__module__.split(".")[0] == "torch":
        if str(dtype) in _TORCH:
            return _TORCH[str(dtype)]
        raise ValueError(f"unsupported element type {dtype}")
    d = np.dtype(dtype)
    for k, v in _NP.items():
        if k != BFLOAT16 and np.dtype(v) == d:
            return k
    raise ValueError(f"unsupported element type {dtype}")


def element_code(dtype) -> int:
    """dtype_code() plus the FP8 types and packed FP4: ``torch.float8_e4m3fn`` is FP8_E4M3,
    ``torch.float8_e5m2`` is FP8_E5M2 and ``torch.float4_e2m1fn_x2`` is FP4_E2M1 (by module and name,
    without importing torch).  numpy has no FP8 or FP4 type, and a plain ``np.uint8`` array is neither
    an FP8 nor an FP4 matrix: pass the code.  Neither numpy nor torch has an FP6 type: FP6_E2M3 and
    FP6_E3M2 are always passed as codes (they pass through), over ``uint8`` storage."""
    if not isinstance(dtype, int) and type(dtype).__module__.split(".")[0] == "torch" \
            and str(dtype) in _TORCH_FP8:
        return _TORCH_FP8[str(dtype)]
    return dtype_code(dtype)


def np_dtype(code: int):
    """numpy type holding one element of ``code``; BFLOAT16 is ``np.uint16`` and the FP8 types are
    ``np.uint8`` (their bits).  FP4_E2M1 is ``np.uint8`` too, but a byte holds TWO elements; FP6_E2M3
    and FP6_E3M2 are ``np.uint8`` as well: 3 bytes hold 4 elements."""
    return _NP_FP8[code] if code in _NP_FP8 else _NP[code]


def _scalar_code(a_code: int, c_code: int) -> int:
    """the type of alpha / beta of an (A, C) pair: C's, FLOAT when A or C is a 2-byte or a 1-byte
    type"""
    return FLOAT if a_code in _FP32_SCALARS or c_code in _FP32_SCALARS else c_code


class _Block(C.Structure):
    _fields_ = [("data", C.c_void_p), ("ld", C.c_int), ("row", C.c_int), ("col", C.c_int)]


_BLOCK_DTYPE = np.dtype([("data", "<u8"), ("ld", "<i4"), ("row", "<i4"), ("col", "<i4")],
                        align=True)
assert _BLOCK_DTYPE.itemsize == C.sizeof(_Block)


class TileOp(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("nf", C.c_int32), ("ns", C.c_int32),
                ("lds", C.c_int32), ("ldd", C.c_int32), ("flags", C.c_uint32),
                ("order", C.c_uint32)]


class TriOp(C.Structure):
    """costa_tri_op_t: element (f, s) of the op is kept when s - f >= diag, or s - f <= diag with
    flag TRI_LE."""
    _fields_ = [("op", TileOp), ("diag", C.c_int32), ("pad", C.c_int32)]


class ScaledOp(C.Structure):
    """costa_scaled_op_t: source element (f, s) of the op is target element (row0 + f, col0 + s)
    with flag SCALED_F_ROWS, (row0 + s, col0 + f) without."""
    _fields_ = [("op", TileOp), ("row0", C.c_int32), ("col0", C.c_int32)]


class DualOp(C.Structure):
    """costa_dual_op_t: the scaled op of output 1 and where source element (f, s) goes in output 2,
    whose element has target coordinates (j, i)."""
    _fields_ = [("s", ScaledOp), ("dst2", C.c_uint64), ("ldd2", C.c_int32), ("flags2", C.c_uint32)]


# MX block-scaled transforms (costa_hip.h): the axis a block of 32 runs along, the rounding of E
MX_ROWS, MX_COLS = 0, 1
MX_FLOOR, MX_CEIL = 0, 1


class MxScales(C.Structure):
    """costa_mx_scales_t: the E8M0 byte of (block b, line l) is data[b*block_stride + l*line_stride];
    axis MX_ROWS: a block is 32 consecutive rows of column l, MX_COLS: 32 consecutive columns of
    row l."""
    _fields_ = [("data", C.c_void_p), ("axis", C.c_int), ("block_stride", C.c_int64),
                ("line_stride", C.c_int64)]

    def __init__(self, data=0, axis=MX_ROWS, block_stride=0, line_stride=0):
        super().__init__(data, axis, block_stride, line_stride)


# Block-scaled FP8 transforms (costa_hip.h): how the fp32 scale of a block is rounded
BLOCK_EXACT, BLOCK_POW2 = 0, 1
BLOCK_SHAPES = ((1, 128), (128, 1), (128, 128))


class BlockScales(C.Structure):
    """costa_block_scales_t: the fp32 scale of block (bi, bj) -- rows bi*block_rows .., columns
    bj*block_cols .. -- is data[bi*row_stride + bj*col_stride] (strides in floats)."""
    _fields_ = [("data", C.c_void_p), ("block_rows", C.c_int32), ("block_cols", C.c_int32),
                ("row_stride", C.c_int64), ("col_stride", C.c_int64)]

    def __init__(self, data=0, block_rows=128, block_cols=128, row_stride=0, col_stride=0):
        super().__init__(data, block_rows, block_cols, row_stride, col_stride)


class PlanInfo(C.Structure):
    _fields_ = [("n_local", C.c_int64), ("n_pack", C.c_int64), ("n_unpack", C.c_int64),
                ("send_elems", C.c_int64), ("recv_elems", C.c_int64),
                ("local_elems", C.c_int64), ("n_ranks", C.c_int32), ("n_slots", C.c_int32)]


class TriPlanInfo(C.Structure):
    _fields_ = [("base", PlanInfo), ("n_local_tri", C.c_int64), ("n_unpack_tri", C.c_int64)]


class ScaledPlanInfo(C.Structure):
    _fields_ = [("base", PlanInfo), ("n_local_scaled", C.c_int64), ("n_unpack_scaled", C.c_int64)]


class Stats(C.Structure):
    _fields_ = [("pack_ms", C.c_double), ("local_ms", C.c_double), ("unpack_ms", C.c_double),
                ("exchange_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double),
                ("pack_launches", C.c_int64), ("local_launches", C.c_int64),
                ("unpack_launches", C.c_int64), ("pack_bytes", C.c_int64),
                ("local_bytes", C.c_int64), ("unpack_bytes", C.c_int64),
                ("transforms", C.c_int64), ("plan_hits", C.c_int64),
                ("plan_misses", C.c_int64), ("host_groups", C.c_int64),
                ("device_plans", C.c_int64), ("plan_ms", C.c_double), ("host_direct", C.c_int64),
                ("host_direct_groups", C.c_int64), ("tile_items", C.c_int64), ("skew_items", C.c_int64),
                ("cblock_items", C.c_int64), ("tiny_items", C.c_int64), ("device_lists", C.c_int64),
                ("fused_pieces", C.c_int64)]

    def as_dict(self) -> dict:
        # (a ctypes subclass lists only the fields it appends: walk the bases first)
        out = {}
        for cls in reversed(type(self).__mro__):
            for k, _ in cls.__dict__.get("_fields_", ()):
                out[k] = getattr(self, k)
        return out


class FullStats(Stats):
    """costa_stats_t as the library fills it: ``Stats`` is its prefix, counters added since are
    appended here in the order of include/costa_hip.h (convert_items: sub-tiles run by the
    converting kernels of mixed-precision transforms; tri_items: sub-tiles run by the edge-tile
    kernels of triangular transforms)."""
    _fields_ = [("convert_items", C.c_int64), ("tri_items", C.c_int64)]


# COSTA_LIB: another build of the library (A/B runs against a tuning build of the sources)
LIB_PATH = os.environ.get("COSTA_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                       "lib", "libcosta_amd.so")
_lib = None


def lib():
    """Load libcosta_amd.so (once).  torch is imported first when available so that the
    process holds ONE HIP runtime (torch's libamdhip64 and the system one share a soname)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.environ.get("COSTA_NO_TORCH"):  # COSTA_NO_TORCH=1: the system HIP / RCCL only
        try:                                      # (tests/rccl_system_child.py)
            import torch  # noqa: F401  (see docstring)
        except Exception:  # pragma: no cover - torch absent is fine for pure C users
            pass
    if not os.path.exists(LIB_PATH):
        raise CostaError(-1, f"native library missing: {LIB_PATH} (run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i, c, i64 = C.c_void_p, C.c_int, C.c_char, C.c_int64
    sig = {
        "costa_hip_last_error": (C.c_char_p, []),
        "costa_hip_version": (i, []),
        "costa_hip_block_cyclic_layout": (i, [i, i, i, i, i, i, i, i, i, i, i, c, i, i, vp, i, c, i,
                                              C.POINTER(vp)]),
        "costa_hip_custom_layout": (i, [i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), i,
                                        C.POINTER(_Block), c, C.POINTER(vp)]),
        "costa_hip_layout_destroy": (None, [vp]),
        "costa_hip_layout_reorder_ranks": (i, [vp, C.POINTER(i), i]),
        "costa_hip_layout_num_blocks": (i, [vp]),
        "costa_hip_layout_shape": (i, [vp, C.POINTER(i), C.POINTER(i)]),
        "costa_hip_layout_block": (i, [vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(i),
                                       C.POINTER(i), C.POINTER(vp), C.POINTER(i)]),
        "costa_hip_comm_self": (i, [i, C.POINTER(vp)]),
        "costa_hip_comm_unique_id": (i, [C.c_char_p]),
        "costa_hip_comm_create": (i, [C.c_char_p, i, i, i, C.POINTER(vp)]),
        "costa_hip_comm_emulated": (i, [i, i, i, C.POINTER(vp)]),
        "costa_hip_comm_emulate": (i, [vp, i, i, vp]),
        "costa_hip_exchange_rounds": (i, []),
        "costa_hip_round_range": (i, [i64, i, i, i, C.POINTER(i64), C.POINTER(i64)]),
        "costa_hip_comm_rank": (i, [vp]),
        "costa_hip_comm_size": (i, [vp]),
        "costa_hip_comm_destroy": (None, [vp]),
        "costa_hip_transform": (i, [vp, vp, c, vp, vp, vp]),
        "costa_hip_transform_batch": (i, [i, C.POINTER(vp), C.POINTER(vp), C.c_char_p, vp, vp,
                                          vp]),
        "costa_hip_transform_async": (i, [vp, vp, c, vp, vp, vp, vp]),
        "costa_hip_transform_batch_async": (i, [i, C.POINTER(vp), C.POINTER(vp), C.c_char_p, vp,
                                                vp, vp, vp]),
        "costa_hip_synchronize": (i, [vp]),
        "costa_hip_device_count": (i, [C.POINTER(i)]),
        "costa_hip_rccl_version": (i, [C.POINTER(i)]),
        "costa_hip_copy_and_transform": (i, [i, i, i, vp, i, i, vp, i, i, i, i, vp, vp]),
        "costa_hip_execute_tiles": (i, [i, C.POINTER(TileOp), i64, vp, vp, vp, i, i]),
        "costa_hip_execute_tiles_mixed": (i, [i, i, C.POINTER(TileOp), i64, vp, vp, vp, i, i]),
        "costa_hip_convert_subtile": (i, [i, i, C.POINTER(i), C.POINTER(i)]),
        "costa_hip_transform_tri": (i, [vp, vp, c, c, i, vp, vp, vp]),
        "costa_hip_transform_tri_async": (i, [vp, vp, c, c, i, vp, vp, vp, vp]),
        "costa_hip_execute_tiles_tri": (i, [i, C.POINTER(TriOp), i64, vp, vp, vp, i, i]),
        "costa_hip_tri_cut": (i, []),
        "costa_hip_tri_phase_ms": (i, [C.POINTER(C.c_double), i]),
        "costa_hip_tri_subtile": (i, [i, C.POINTER(i), C.POINTER(i)]),
        "costa_hip_plan_export_tri": (i, [vp, vp, c, c, i, vp, vp, i, i, C.POINTER(TriPlanInfo), vp, vp,
                                          vp, vp, vp, vp, vp, vp, vp, vp]),
        "costa_hip_transform_scaled": (i, [vp, vp, c, vp, vp, vp, vp, vp]),
        "costa_hip_transform_scaled_async": (i, [vp, vp, c, vp, vp, vp, vp, vp, vp]),
        "costa_hip_execute_tiles_scaled": (i, [i, i, C.POINTER(ScaledOp), i64, vp, vp, vp, i, vp, vp, i]),
        "costa_hip_scaled_subtile": (i, [i, i, C.POINTER(i), C.POINTER(i)]),
        "costa_hip_mx_subtile": (i, [i, i, C.POINTER(i), C.POINTER(i)]),
        "costa_hip_block_subtile": (i, [i, i, C.POINTER(i), C.POINTER(i)]),
        "costa_hip_scaled_items": (i, [C.POINTER(i64), i]),
        "costa_hip_transform_amax": (i, [vp, vp, c, vp, vp, vp, vp, vp, vp, vp]),
        "costa_hip_transform_amax_async": (i, [vp, vp, c, vp, vp, vp, vp, vp, vp, vp, vp]),
        "costa_hip_layout_amax": (i, [vp, vp, vp, vp]),
        "costa_hip_layout_amax_async": (i, [vp, vp, vp, vp, vp]),
        "costa_hip_execute_tiles_amax": (i, [i, i, C.POINTER(ScaledOp), i64, vp, vp, vp, i, vp, vp, vp, vp,
                                             i]),
        "costa_hip_amax_items": (i, [C.POINTER(i64), i]),
        "costa_hip_transform_mx": (i, [vp, vp, c, vp, vp, C.POINTER(MxScales), C.POINTER(MxScales), i, vp]),
        "costa_hip_transform_mx_async": (i, [vp, vp, c, vp, vp, C.POINTER(MxScales), C.POINTER(MxScales), i,
                                             vp, vp]),
        "costa_hip_execute_tiles_mx": (i, [i, i, C.POINTER(ScaledOp), i64, vp, vp, vp, i, C.POINTER(MxScales),
                                           C.POINTER(MxScales), i, i64, i64, i, i]),
        "costa_hip_mx_items": (i, [C.POINTER(i64), i]),
        "costa_hip_transform_mx_sr": (i, [vp, vp, c, vp, vp, C.POINTER(MxScales), C.POINTER(MxScales), i,
                                          C.c_uint64, vp]),
        "costa_hip_transform_mx_sr_async": (i, [vp, vp, c, vp, vp, C.POINTER(MxScales), C.POINTER(MxScales), i,
                                                C.c_uint64, vp, vp]),
        "costa_hip_execute_tiles_mx_sr": (i, [i, i, C.POINTER(ScaledOp), i64, vp, vp, vp, i,
                                              C.POINTER(MxScales), C.POINTER(MxScales), i, i64, i64, i,
                                              C.c_uint64, i]),
        "costa_hip_sr_bits": (i, [C.c_uint64, i64, i64, C.POINTER(C.c_uint32)]),
        "costa_hip_transform_mx_dual": (i, [vp, vp, vp, c, vp, C.POINTER(MxScales), C.POINTER(MxScales), i,
                                            C.POINTER(C.c_uint64), vp]),
        "costa_hip_transform_mx_dual_async": (i, [vp, vp, vp, c, vp, C.POINTER(MxScales), C.POINTER(MxScales),
                                                  i, C.POINTER(C.c_uint64), vp, vp]),
        "costa_hip_execute_tiles_mx_dual": (i, [i, C.POINTER(DualOp), i64, vp, vp, vp, vp, i,
                                                C.POINTER(MxScales), C.POINTER(MxScales), i, i64, i64,
                                                C.POINTER(C.c_uint64), i]),
        "costa_hip_mx_dual_items": (i, [C.POINTER(i64), i]),
        "costa_hip_plan_export_dual": (i, [vp, vp, vp, c, vp, i, i, i, i, C.POINTER(ScaledPlanInfo), vp, vp]),
        "costa_hip_transform_block_scaled": (i, [vp, vp, c, vp, vp, C.POINTER(BlockScales),
                                                 C.POINTER(BlockScales), i, vp]),
        "costa_hip_transform_block_scaled_async": (i, [vp, vp, c, vp, vp, C.POINTER(BlockScales),
                                                       C.POINTER(BlockScales), i, vp, vp]),
        "costa_hip_execute_tiles_block_scaled": (i, [i, i, C.POINTER(ScaledOp), i64, vp, vp, vp, i,
                                                     C.POINTER(BlockScales), C.POINTER(BlockScales), i, i64,
                                                     i64, i, i]),
        "costa_hip_block_items": (i, [C.POINTER(i64), i]),
        "costa_hip_block_check_ops": (i, [C.POINTER(ScaledOp), i64, i, i, i64, i64]),
        "costa_hip_block_check_scales": (i, [C.POINTER(BlockScales), i64, i64]),
        "costa_hip_mx_check_ops": (i, [C.POINTER(ScaledOp), i64, i, i64, i64]),
        "costa_hip_mx_check_scales": (i, [C.POINTER(MxScales), i64, i64]),
        "costa_hip_plan_export_scaled": (i, [vp, vp, c, vp, vp, i, i, C.POINTER(ScaledPlanInfo), vp, vp,
                                             vp, vp, vp, vp, vp, vp]),
        "costa_hip_plan_export": (i, [i, C.POINTER(vp), C.POINTER(vp), C.c_char_p, vp, vp, i, i,
                                      C.POINTER(PlanInfo), vp, vp, vp, vp, vp, vp, vp, vp]),
        "costa_hip_set_profiling": (i, [i]),
        "costa_hip_get_stats": (i, [C.POINTER(FullStats), i]),
        "costa_hip_release_caches": (i, []),
        "costa_hip_set_host_staging": (i, [i]),
        "costa_hip_set_planner": (i, [i]),
        "costa_hip_plan_export_device": (i, [i, i, C.POINTER(vp), C.POINTER(vp), C.c_char_p, vp, vp,
                                             i, i, C.POINTER(PlanInfo), vp, vp, vp, vp, vp, vp, vp,
                                             vp]),
        "costa_hip_set_list_builder": (i, [i]),
        "costa_hip_work_export": (i, [i, vp, i64, i, i, vp, i64, vp, i64, C.POINTER(i64)]),
    }
    for name, (res, args) in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            # an older build selected with COSTA_LIB for an A/B run lacks the newer entry points:
            # calling one raises AttributeError; the package's own library must have them all
            if os.environ.get("COSTA_LIB"):
                continue
            raise
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise CostaError(rc, lib().costa_hip_last_error().decode(errors="replace"))


def _ptr(p) -> int:
    """Accept an int address, a numpy array, or anything with data_ptr() (torch tensor)."""
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    if isinstance(p, np.ndarray):
        return p.ctypes.data
    if hasattr(p, "data_ptr"):
        return p.data_ptr()
    raise TypeError(f"cannot take the address of {type(p)}")


def _scalar_bytes(code: int, x) -> bytes:
    if code in _FP32_SCALARS:  # the scalars of half-precision and FP8 transforms are fp32
        code = FLOAT
    if code == DOUBLE:
        return struct.pack("<d", float(x))
    if code == CDOUBLE:
        z = complex(x)
        return struct.pack("<dd", z.real, z.imag)
    return np.asarray(x, dtype=_NP[code]).reshape(1).tobytes()


def _chr(x: str) -> C.c_char:
    return C.c_char(x.encode()[:1])


# ------------------------------------------------------------------ layouts
@dataclass
class BlockInfo:
    row_start: int
    row_end: int
    col_start: int
    col_end: int
    data: int
    ld: int


class Layout:
    """Handle of a native grid_layout (reference grid_layout.hpp:8-189).  Holds references to
    the Python objects owning the memory so they outlive the layout."""

    def __init__(self, handle: int, dtype: int, keep: Iterable = ()):
        self._h = C.c_void_p(handle)
        self.dtype = dtype
        self._keep = list(keep)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def num_blocks(self) -> int:
        return lib().costa_hip_layout_num_blocks(self._h)

    def block(self, i: int) -> BlockInfo:
        v = [C.c_int() for _ in range(4)]
        d, ld = C.c_void_p(), C.c_int()
        _check(lib().costa_hip_layout_block(self._h, i, *[C.byref(x) for x in v], C.byref(d),
                                            C.byref(ld)))
        return BlockInfo(v[0].value, v[1].value, v[2].value, v[3].value, d.value or 0, ld.value)

    def shape(self) -> tuple:
        """(m, n) of the matrix the layout describes (costa_hip_layout_shape)."""
        m, n = C.c_int(), C.c_int()
        _check(lib().costa_hip_layout_shape(self._h, C.byref(m), C.byref(n)))
        return m.value, n.value

    def reorder_ranks(self, reordering: Sequence[int]):
        """Rank relabelling: owner(i, j) -> reordering[owner(i, j)] (reference
        grid_layout::reorder_ranks, grid_layout.hpp:32-34)."""
        p = np.ascontiguousarray(reordering, dtype=np.int32)
        _check(lib().costa_hip_layout_reorder_ranks(self._h, p.ctypes.data_as(C.POINTER(C.c_int)),
                                                    int(p.size)))

    def close(self):
        if self._h and self._h.value:
            lib().costa_hip_layout_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def block_cyclic_layout(m, n, block_m, block_n, i, j, sub_m, sub_n, p_m, p_n, order, rsrc, csrc,
                        ptr, lld, ordering, rank, dtype=DOUBLE) -> Layout:
    """ScaLAPACK block-cyclic layout of sub(A) (reference layout.hpp:70-86)."""
    code = element_code(dtype)
    h = C.c_void_p()
    _check(lib().costa_hip_block_cyclic_layout(code, m, n, block_m, block_n, i, j, sub_m, sub_n,
                                               p_m, p_n, _chr(order), rsrc, csrc,
                                               C.c_void_p(_ptr(ptr)), lld, _chr(ordering), rank,
                                               C.byref(h)))
    return Layout(h.value, code, [ptr])


def custom_layout(rowblocks, colblocks, rowsplit, colsplit, owners, localblocks, ordering,
                  dtype=DOUBLE) -> Layout:
    """Arbitrary grid layout (reference layout.hpp:34-42).  ``localblocks`` is a sequence of
    (data, ld, row, col) with data an address/array/tensor."""
    code = element_code(dtype)
    rs = np.ascontiguousarray(rowsplit, dtype=np.int32)
    cs = np.ascontiguousarray(colsplit, dtype=np.int32)
    ow = np.ascontiguousarray(owners, dtype=np.int32).reshape(-1)
    lb = list(localblocks)
    # numpy image of costa_block_t[] (built column-wise: ~100x faster than ctypes structs)
    arr = np.zeros(max(1, len(lb)), _BLOCK_DTYPE)
    if lb:
        arr["data"][:len(lb)] = [_ptr(b[0]) for b in lb]
        rest = np.asarray([b[1:4] for b in lb], dtype=np.int64).reshape(len(lb), 3)
        arr["ld"][:len(lb)] = rest[:, 0]
        arr["row"][:len(lb)] = rest[:, 1]
        arr["col"][:len(lb)] = rest[:, 2]
    h = C.c_void_p()
    ip = C.POINTER(C.c_int)
    _check(lib().costa_hip_custom_layout(code, rowblocks, colblocks, rs.ctypes.data_as(ip),
                                         cs.ctypes.data_as(ip), ow.ctypes.data_as(ip), len(lb),
                                         arr.ctypes.data_as(C.POINTER(_Block)), _chr(ordering),
                                         C.byref(h)))
    return Layout(h.value, code, [b[0] for b in lb])


# ------------------------------------------------------------------ communicators
EMULATE_PACK, EMULATE_UNPACK, EMULATE_LOCAL = 1, 2, 3
EMULATE_PARTS = {"pack": EMULATE_PACK, "unpack": EMULATE_UNPACK, "local": EMULATE_LOCAL}


def exchange_rounds() -> int:
    """Parts a peer's package of at least 16 MiB is exchanged in (costa_hip_exchange_rounds)."""
    return lib().costa_hip_exchange_rounds()


def round_range(count: int, elem_bytes: int, rounds: int, round: int) -> tuple:
    """Element range [lo, hi) that round ``round`` of ``rounds`` moves of a package of ``count``
    elements of ``elem_bytes`` bytes (costa_hip_round_range; host only)."""
    lo, hi = C.c_int64(), C.c_int64()
    _check(lib().costa_hip_round_range(count, elem_bytes, rounds, round, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


class Comm:
    """One rank per GPU.  ``Comm.self(device)`` for a single rank; for several ranks one rank
    calls ``Comm.unique_id()``, the caller broadcasts the 128 bytes, and every rank calls
    ``Comm.create(uid, nranks, rank, device)`` (collective)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    @staticmethod
    def self(device: int = 0) -> "Comm":
        h = C.c_void_p()
        _check(lib().costa_hip_comm_self(device, C.byref(h)))
        return Comm(h.value)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().costa_hip_comm_unique_id(buf))
        return buf.raw

    @staticmethod
    def create(uid: bytes, nranks: int, rank: int, device: int) -> "Comm":
        assert len(uid) == 128
        h = C.c_void_p()
        _check(lib().costa_hip_comm_create(uid, nranks, rank, device, C.byref(h)))
        return Comm(h.value)

    @staticmethod
    def emulated(rank: int, nranks: int, device: int = 0) -> "Comm":
        """Test mode: rank ``rank`` of ``nranks`` without RCCL, planned like an RCCL communicator of
        that size; ``emulate`` selects the part its transforms launch (costa_hip.h, "test modes")."""
        h = C.c_void_p()
        _check(lib().costa_hip_comm_emulated(rank, nranks, device, C.byref(h)))
        return Comm(h.value)

    def emulate(self, part, round: int = -1, buffer=None):
        """The part the next transforms on this emulated communicator launch: ``"pack"`` /
        ``"unpack"`` round ``round`` (-1: every round) into / from the package ``buffer``, or
        ``"local"``."""
        code = EMULATE_PARTS.get(part, part) if isinstance(part, str) else int(part)
        _check(lib().costa_hip_comm_emulate(self._h, code, round, C.c_void_p(_ptr(buffer))))

    @property
    def handle(self):
        return self._h

    @property
    def rank(self) -> int:
        return lib().costa_hip_comm_rank(self._h)

    @property
    def size(self) -> int:
        return lib().costa_hip_comm_size(self._h)

    def close(self):
        if self._h and self._h.value:
            lib().costa_hip_comm_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ transforms
def transform(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", alpha=1, beta=0):
    """sub(C) = beta*sub(C) + alpha*op(sub(A)) (reference transform.hpp:13-27).

    A and C may differ in dtype (FLOAT <-> DOUBLE, CFLOAT <-> CDOUBLE; device-resident layouts):
    sub(A) is converted to C's type inside the tile kernels, and alpha / beta are of C's type
    (costa_hip.h, "Mixed precision").  HALF / BFLOAT16 layouts pair with themselves and with FLOAT
    (H -> H, FLOAT -> H, H -> FLOAT): fp32 arithmetic with one rounding at the store, alpha / beta
    fp32 (costa_hip.h, "Half precision").  FP8_E4M3 / FP8_E5M2 layouts pair the same way (Q -> Q,
    FLOAT -> Q, Q -> FLOAT); a FLOAT source is not rounded before the arithmetic, so FLOAT -> Q
    with alpha = 1 / scale quantises (costa_hip.h, "FP8")."""
    transform_batch([A], [Cl], comm, [trans], [alpha], [beta])


def transform_batch(As: Sequence[Layout], Cs: Sequence[Layout], comm: Comm,
                    trans: Sequence[str] | None = None, alpha=None, beta=None):
    """Several layout pairs in one exchange (reference transform.hpp:38-43)."""
    n = len(As)
    assert n == len(Cs) and n > 0
    code = _scalar_code(As[0].dtype, Cs[0].dtype)  # alpha / beta: C's type (half pairs: fp32)
    trans = list(trans) if trans is not None else ["N"] * n
    alpha = list(alpha) if alpha is not None else [1] * n
    beta = list(beta) if beta is not None else [0] * n
    a = (C.c_void_p * n)(*[x.handle.value for x in As])
    c = (C.c_void_p * n)(*[x.handle.value for x in Cs])
    ab = b"".join(_scalar_bytes(code, x) for x in alpha)
    bb = b"".join(_scalar_bytes(code, x) for x in beta)
    _check(lib().costa_hip_transform_batch(n, a, c, "".join(trans).encode(), ab, bb, comm.handle))


def transform_async(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", alpha=1, beta=0,
                    stream=None):
    """Stream-ordered transform (device-resident layouts).  `stream`: a torch stream, a raw
    hipStream_t address, or None; it waits for the result.  See costa_hip_transform_async."""
    transform_batch_async([A], [Cl], comm, [trans], [alpha], [beta], stream)


def transform_batch_async(As, Cs, comm: Comm, trans=None, alpha=None, beta=None, stream=None):
    n = len(As)
    code = _scalar_code(As[0].dtype, Cs[0].dtype)  # alpha / beta: C's type (half pairs: fp32)
    trans = list(trans) if trans is not None else ["N"] * n
    alpha = list(alpha) if alpha is not None else [1] * n
    beta = list(beta) if beta is not None else [0] * n
    a = (C.c_void_p * n)(*[x.handle.value for x in As])
    c = (C.c_void_p * n)(*[x.handle.value for x in Cs])
    ab = b"".join(_scalar_bytes(code, x) for x in alpha)
    bb = b"".join(_scalar_bytes(code, x) for x in beta)
    s = getattr(stream, "cuda_stream", stream) or 0
    _check(lib().costa_hip_transform_batch_async(n, a, c, "".join(trans).encode(), ab, bb,
                                                 comm.handle, C.c_void_p(s)))


def synchronize(comm: Comm):
    """Wait for every transform queued on the communicator's device."""
    _check(lib().costa_hip_synchronize(comm.handle))


class transformer:
    """Batches layout pairs into one exchange (reference transformer.hpp:8-62)."""

    def __init__(self, comm: Comm):
        self.comm = comm
        self.clear()

    def schedule(self, A: Layout, Cl: Layout, trans: str | None = None, alpha=None, beta=None):
        self.frm.append(A)
        self.to.append(Cl)
        if trans is not None:
            self.trans.append(trans)
            self.alpha.append(alpha)
            self.beta.append(beta)

    def transform(self):
        if self.alpha and len(self.alpha) != len(self.frm):
            raise ValueError("mix of scaled and unscaled schedule() calls")
        if self.alpha:
            transform_batch(self.frm, self.to, self.comm, self.trans, self.alpha, self.beta)
        else:
            transform_batch(self.frm, self.to, self.comm)
        self.clear()

    def clear(self):
        self.frm, self.to, self.trans, self.alpha, self.beta = [], [], [], [], []


def copy_and_transform(dtype, n_rows, n_cols, src, src_stride, src_col_major, dst, dst_stride,
                       dst_col_major, transpose=False, conjugate=False, alpha=1, beta=0):
    """One tile on device pointers (reference memory_utils.hpp:339-412)."""
    code = element_code(dtype)
    _check(lib().costa_hip_copy_and_transform(
        code, n_rows, n_cols, C.c_void_p(_ptr(src)), src_stride, int(bool(src_col_major)),
        C.c_void_p(_ptr(dst)), dst_stride, int(bool(dst_col_major)), int(bool(transpose)),
        int(bool(conjugate)), _scalar_bytes(code, alpha), _scalar_bytes(code, beta)))


def execute_tiles(dtype, ops: np.ndarray, scalars: np.ndarray, src_base=0, dst_base=0,
                  device: int = 0):
    """Run a tile-op list (numpy array of TILE_OP_DTYPE) in one batched launch."""
    code = element_code(dtype)
    ops = np.ascontiguousarray(ops, dtype=TILE_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=np_dtype(code)).reshape(-1)
    assert sc.size % 2 == 0
    _check(lib().costa_hip_execute_tiles(code, ops.ctypes.data_as(C.POINTER(TileOp)), ops.size,
                                         C.c_void_p(_ptr(src_base)), C.c_void_p(_ptr(dst_base)),
                                         sc.ctypes.data, sc.size // 2, device))


def execute_tiles_mixed(src_dtype, dst_dtype, ops: np.ndarray, scalars: np.ndarray, src_base=0,
                        dst_base=0, device: int = 0):
    """Run a list of converting tile ops (sources of ``src_dtype``, destinations of ``dst_dtype``:
    FLOAT <-> DOUBLE or CFLOAT <-> CDOUBLE) in one batched launch; ``scalars`` are of
    ``dst_dtype`` (costa_hip_execute_tiles_mixed).  Half-precision pairs ((H, H), (FLOAT, H),
    (H, FLOAT) with H = HALF or BFLOAT16) and FP8 pairs (the same shapes with FP8_E4M3 or FP8_E5M2)
    run here too, with fp32 ``scalars``."""
    sc_, dc_ = element_code(src_dtype), element_code(dst_dtype)
    ops = np.ascontiguousarray(ops, dtype=TILE_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=_NP[_scalar_code(sc_, dc_)]).reshape(-1)
    assert sc.size % 2 == 0
    _check(lib().costa_hip_execute_tiles_mixed(sc_, dc_, ops.ctypes.data_as(C.POINTER(TileOp)),
                                               ops.size, C.c_void_p(_ptr(src_base)),
                                               C.c_void_p(_ptr(dst_base)), sc.ctypes.data,
                                               sc.size // 2, device))


def convert_subtile(src_dtype, dst_dtype) -> tuple:
    """(BF, BS): the sub-tile of the converting kernels for a mixed pair, in elements along the
    source's fast and slow dimension (one workgroup each)."""
    bf, bs = C.c_int(0), C.c_int(0)
    _check(lib().costa_hip_convert_subtile(element_code(src_dtype), element_code(dst_dtype),
                                           C.byref(bf), C.byref(bs)))
    return bf.value, bs.value


# ------------------------------------------------------------------ triangular transforms
def _one_pair(A, Cl):
    if not isinstance(A, Layout) or not isinstance(Cl, Layout):
        raise CostaError(1, "costa: batches of triangular (masked) layout pairs are not supported")


def transform_tri(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", uplo: str = "U", k: int = 0,
                  alpha=1, beta=0):
    """C(i, j) = beta*C(i, j) + alpha*op(A)(i, j) where j - i >= k (uplo 'U', numpy triu(k)) or
    j - i <= k ('L', tril(k)); every other element of C keeps its bytes (costa_hip_transform_tri)."""
    _one_pair(A, Cl)
    code = Cl.dtype
    _check(lib().costa_hip_transform_tri(A.handle, Cl.handle, _chr(trans), _chr(uplo), int(k),
                                         _scalar_bytes(code, alpha), _scalar_bytes(code, beta),
                                         comm.handle))


def transform_tri_async(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", uplo: str = "U",
                        k: int = 0, alpha=1, beta=0, stream=None):
    """Stream-ordered transform_tri (device-resident layouts); `stream` as for transform_async."""
    _one_pair(A, Cl)
    code = Cl.dtype
    s = getattr(stream, "cuda_stream", stream) or 0
    _check(lib().costa_hip_transform_tri_async(A.handle, Cl.handle, _chr(trans), _chr(uplo), int(k),
                                               _scalar_bytes(code, alpha), _scalar_bytes(code, beta),
                                               comm.handle, C.c_void_p(s)))


def execute_tiles_tri(dtype, ops: np.ndarray, scalars: np.ndarray, src_base=0, dst_base=0,
                      device: int = 0):
    """Run a list of edge ops (numpy array of TRI_OP_DTYPE) in one launch of the edge-tile kernel."""
    code = element_code(dtype)
    ops = np.ascontiguousarray(ops, dtype=TRI_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=np_dtype(code)).reshape(-1)
    assert sc.size % 2 == 0
    _check(lib().costa_hip_execute_tiles_tri(code, ops.ctypes.data_as(C.POINTER(TriOp)), ops.size,
                                             C.c_void_p(_ptr(src_base)), C.c_void_p(_ptr(dst_base)),
                                             sc.ctypes.data, sc.size // 2, device))


def tri_cut() -> int:
    """Rows of the bands the planner cuts a tile crossing the mask's diagonal into."""
    return lib().costa_hip_tri_cut()


def tri_phase_ms(reset: bool = False) -> float:
    """Event time (ms, profiling on) of the edge-tile launches since the last reset: a part of the
    statistics' local_ms + unpack_ms."""
    v = C.c_double(0)
    _check(lib().costa_hip_tri_phase_ms(C.byref(v), int(reset)))
    return v.value


def tri_subtile(dtype) -> tuple:
    """(BF, BS): the sub-tile one workgroup of the edge-tile kernel runs, in elements along the
    source's fast and slow dimension."""
    bf, bs = C.c_int(0), C.c_int(0)
    _check(lib().costa_hip_tri_subtile(element_code(dtype), C.byref(bf), C.byref(bs)))
    return bf.value, bs.value


@dataclass
class Plan:
    local_ops: np.ndarray
    pack_ops: np.ndarray
    unpack_ops: np.ndarray
    send_counts: np.ndarray
    send_displs: np.ndarray
    recv_counts: np.ndarray
    recv_displs: np.ndarray
    scalars: np.ndarray
    send_elems: int
    recv_elems: int
    local_elems: int


def plan_export(As: Sequence[Layout], Cs: Sequence[Layout], rank: int, nranks: int,
                trans=None, alpha=None, beta=None, device=None) -> Plan:
    """Tile-op lists of `rank`: by the host planner (never touches a GPU), or with ``device``
    set by the GPU planner of that device (costa_hip_plan_export_device)."""
    n = len(As)
    code = _scalar_code(As[0].dtype, Cs[0].dtype)  # alpha / beta: C's type (half pairs: fp32)
    trans = list(trans) if trans is not None else ["N"] * n
    alpha = list(alpha) if alpha is not None else [1] * n
    beta = list(beta) if beta is not None else [0] * n
    a = (C.c_void_p * n)(*[x.handle.value for x in As])
    c = (C.c_void_p * n)(*[x.handle.value for x in Cs])
    ab = b"".join(_scalar_bytes(code, x) for x in alpha)
    bb = b"".join(_scalar_bytes(code, x) for x in beta)
    tb = "".join(trans).encode()
    info = PlanInfo()
    L = lib()
    if device is None:
        export = L.costa_hip_plan_export
    else:
        def export(*args):
            return L.costa_hip_plan_export_device(int(device), *args)
    _check(export(n, a, c, tb, ab, bb, rank, nranks, C.byref(info), None, None,
                  None, None, None, None, None, None))
    lo = np.zeros(info.n_local, TILE_OP_DTYPE)
    po = np.zeros(info.n_pack, TILE_OP_DTYPE)
    uo = np.zeros(info.n_unpack, TILE_OP_DTYPE)
    cnt = [np.zeros(nranks, np.int64) for _ in range(4)]
    sc = np.zeros(2 * info.n_slots, _NP[code])
    _check(export(n, a, c, tb, ab, bb, rank, nranks, C.byref(info),
                  lo.ctypes.data, po.ctypes.data, uo.ctypes.data,
                  *[x.ctypes.data for x in cnt], sc.ctypes.data))
    return Plan(lo, po, uo, *cnt, sc, info.send_elems, info.recv_elems, info.local_elems)


@dataclass
class TriPlan(Plan):
    local_tri: np.ndarray = None   # TRI_OP_DTYPE: edge tiles that stay on the rank
    unpack_tri: np.ndarray = None  # TRI_OP_DTYPE: edge tiles read from the receive package


def plan_export_tri(A: Layout, Cl: Layout, rank: int, nranks: int, trans: str = "N", uplo: str = "U",
                    k: int = 0, alpha=1, beta=0) -> TriPlan:
    """Tile-op lists of `rank` for a triangular transform (host planner, never touches a GPU)."""
    _one_pair(A, Cl)
    code = Cl.dtype
    ab, bb = _scalar_bytes(code, alpha), _scalar_bytes(code, beta)
    info = TriPlanInfo()
    L = lib()
    args = (A.handle, Cl.handle, _chr(trans), _chr(uplo), int(k), ab, bb, rank, nranks, C.byref(info))
    _check(L.costa_hip_plan_export_tri(*args, *([None] * 10)))
    b = info.base
    lo = np.zeros(b.n_local, TILE_OP_DTYPE)
    po = np.zeros(b.n_pack, TILE_OP_DTYPE)
    uo = np.zeros(b.n_unpack, TILE_OP_DTYPE)
    lt = np.zeros(info.n_local_tri, TRI_OP_DTYPE)
    ut = np.zeros(info.n_unpack_tri, TRI_OP_DTYPE)
    cnt = [np.zeros(nranks, np.int64) for _ in range(4)]
    sc = np.zeros(2 * b.n_slots, _NP[code])
    _check(L.costa_hip_plan_export_tri(*args, lo.ctypes.data, po.ctypes.data, uo.ctypes.data,
                                       lt.ctypes.data, ut.ctypes.data, *[x.ctypes.data for x in cnt],
                                       sc.ctypes.data))
    return TriPlan(lo, po, uo, *cnt, sc, b.send_elems, b.recv_elems, b.local_elems, lt, ut)


# ------------------------------------------------------------------ scaled transforms
def _scale_arg(v, code: int, count: int, what: str) -> int:
    """Address of a scale vector: None, a raw device address, or a torch CUDA tensor, which is
    checked against the compute type, for contiguity and for its length."""
    if v is None:
        return 0
    if isinstance(v, int):
        return v
    if type(v).__module__.split(".")[0] != "torch":
        raise ValueError(f"{what}: a torch CUDA tensor or a raw device address, not {type(v)}")
    if not v.is_cuda:
        raise ValueError(f"{what}: the tensor must be device-resident (a CUDA tensor)")
    if dtype_code(v.dtype) != code:
        raise ValueError(f"{what}: dtype {v.dtype}, the compute type is {np.dtype(_NP[code]).name}")
    if not v.is_contiguous():
        raise ValueError(f"{what}: the tensor must be contiguous")
    if v.numel() != count:
        raise ValueError(f"{what}: {v.numel()} elements, the matrix has {count}")
    return v.data_ptr()


def transform_scaled(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", alpha=1, beta=0,
                     row_scale=None, col_scale=None, stream=None):
    """C(i, j) = beta*C(i, j) + alpha*((op(A)(i, j) * row_scale[i]) * col_scale[j]), the scale
    vectors fused into the tile kernels (costa_hip_transform_scaled).  ``row_scale`` (m elements)
    and ``col_scale`` (n elements; m x n the matrix C's layout describes) are torch CUDA tensors or
    raw device addresses of the compute type (float32; float64 for DOUBLE layouts); either may be
    None, not both.  A tensor is checked for dtype, contiguity and length (ValueError).  With
    ``stream`` (a torch stream or a raw hipStream_t address) the call is stream-ordered
    (costa_hip_transform_scaled_async) and the vectors must stay valid until the stream has passed
    it.  A and C may be the same layout when trans is 'N' (in place)."""
    if not isinstance(A, Layout) or not isinstance(Cl, Layout):
        raise CostaError(1, "costa: batches of scaled layout pairs are not supported")
    code = _scalar_code(A.dtype, Cl.dtype)
    m, n = Cl.shape()
    rp = _scale_arg(row_scale, code, m, "row_scale")
    cp = _scale_arg(col_scale, code, n, "col_scale")
    ab, bb = _scalar_bytes(code, alpha), _scalar_bytes(code, beta)
    if stream is None:
        _check(lib().costa_hip_transform_scaled(A.handle, Cl.handle, _chr(trans), ab, bb,
                                                C.c_void_p(rp), C.c_void_p(cp), comm.handle))
    else:
        s = getattr(stream, "cuda_stream", stream) or 0
        _check(lib().costa_hip_transform_scaled_async(A.handle, Cl.handle, _chr(trans), ab, bb,
                                                      C.c_void_p(rp), C.c_void_p(cp), comm.handle,
                                                      C.c_void_p(s)))


def execute_tiles_scaled(src_dtype, dst_dtype, ops: np.ndarray, scalars: np.ndarray, src_base=0,
                         dst_base=0, row_scale=None, col_scale=None, device: int = 0):
    """Run a list of scaled ops (numpy array of SCALED_OP_DTYPE) in one launch of the scaled kernel;
    ``scalars`` are of the compute type, the scale vectors device arrays of it indexed by the ops'
    target coordinates (costa_hip_execute_tiles_scaled)."""
    sc_, dc_ = element_code(src_dtype), element_code(dst_dtype)
    ops = np.ascontiguousarray(ops, dtype=SCALED_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=_NP[_scalar_code(sc_, dc_)]).reshape(-1)
    assert sc.size % 2 == 0
    _check(lib().costa_hip_execute_tiles_scaled(sc_, dc_, ops.ctypes.data_as(C.POINTER(ScaledOp)),
                                                ops.size, C.c_void_p(_ptr(src_base)),
                                                C.c_void_p(_ptr(dst_base)), sc.ctypes.data,
                                                sc.size // 2, C.c_void_p(_ptr(row_scale)),
                                                C.c_void_p(_ptr(col_scale)), device))


def scaled_subtile(src_dtype, dst_dtype) -> tuple:
    """(BF, BS): the sub-tile one workgroup of the scaled kernel runs for an accepted pair."""
    bf, bs = C.c_int(0), C.c_int(0)
    _check(lib().costa_hip_scaled_subtile(element_code(src_dtype), element_code(dst_dtype),
                                          C.byref(bf), C.byref(bs)))
    return bf.value, bs.value


def mx_subtile(src_dtype, dst_dtype) -> tuple:
    """(bf, bs) of the sub-tile one workgroup runs for an MX pair (costa_hip_mx_subtile)"""
    bf, bs = C.c_int(), C.c_int()
    _check(lib().costa_hip_mx_subtile(element_code(src_dtype), element_code(dst_dtype), C.byref(bf), C.byref(bs)))
    return bf.value, bs.value


def block_subtile(src_dtype, dst_dtype) -> tuple:
    """(bf, bs) of the sub-tile (a quantising pair: the region) one workgroup runs for a block-scaled
    pair (costa_hip_block_subtile)"""
    bf, bs = C.c_int(), C.c_int()
    _check(lib().costa_hip_block_subtile(element_code(src_dtype), element_code(dst_dtype), C.byref(bf), C.byref(bs)))
    return bf.value, bs.value


def scaled_items(reset: bool = False) -> int:
    """Sub-tiles run by the scaled kernel since the last reset."""
    v = C.c_int64(0)
    _check(lib().costa_hip_scaled_items(C.byref(v), int(reset)))
    return v.value


# ------------------------------------------------------------------ amax outputs
def transform_amax(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", alpha=1, beta=0,
                   row_scale=None, col_scale=None, row_amax=None, col_amax=None, stream=None):
    """``transform_scaled`` with the same arguments (here both scales may be None: both products are
    skipped) that also updates ``row_amax[i]`` / ``col_amax[j]`` (m / n elements of the compute
    type, at least one given) with the abs-max, taken as an unsigned maximum of bit patterns, over the
    elements (i, j) of C this rank writes; x is the source value before the scales and alpha / beta
    (costa_hip_transform_amax; costa_hip.h, "amax outputs").  The update accumulates: initialise the
    vectors, normally with zeros; entries must be non-negative on entry.  Amax vectors are torch
    CUDA tensors, checked like the scale tensors (ValueError), or raw device addresses (unchecked).
    With several ranks each rank's vectors cover its own part of C: max-reduce them across ranks."""
    if not isinstance(A, Layout) or not isinstance(Cl, Layout):
        raise CostaError(1, "costa: batches of scaled layout pairs are not supported")
    code = _scalar_code(A.dtype, Cl.dtype)
    m, n = Cl.shape()
    rp = _scale_arg(row_scale, code, m, "row_scale")
    cp = _scale_arg(col_scale, code, n, "col_scale")
    ra = _scale_arg(row_amax, code, m, "row_amax")
    ca = _scale_arg(col_amax, code, n, "col_amax")
    ab, bb = _scalar_bytes(code, alpha), _scalar_bytes(code, beta)
    args = (A.handle, Cl.handle, _chr(trans), ab, bb, C.c_void_p(rp), C.c_void_p(cp), C.c_void_p(ra),
            C.c_void_p(ca), comm.handle)
    if stream is None:
        _check(lib().costa_hip_transform_amax(*args))
    else:
        s = getattr(stream, "cuda_stream", stream) or 0
        _check(lib().costa_hip_transform_amax_async(*args, C.c_void_p(s)))


def layout_amax(A: Layout, comm: Comm, row_amax=None, col_amax=None, stream=None):
    """Update ``row_amax`` / ``col_amax`` (rows / columns of the matrix A's layout describes; float32,
    float64 for DOUBLE layouts; at least one given) with the abs-max of A's local blocks, whatever
    their padding and ordering: a reduce-only pass that writes nothing else (costa_hip_layout_amax).
    FLOAT, DOUBLE, HALF, BFLOAT16 and FP8 layouts on the device.  The vectors accumulate and are
    checked as in ``transform_amax``; with ``stream`` the call is stream-ordered."""
    if not isinstance(A, Layout):
        raise CostaError(1, "costa: layout_amax takes one layout")
    code = DOUBLE if A.dtype == DOUBLE else FLOAT
    m, n = A.shape()
    ra = _scale_arg(row_amax, code, m, "row_amax")
    ca = _scale_arg(col_amax, code, n, "col_amax")
    if stream is None:
        _check(lib().costa_hip_layout_amax(A.handle, C.c_void_p(ra), C.c_void_p(ca), comm.handle))
    else:
        s = getattr(stream, "cuda_stream", stream) or 0
        _check(lib().costa_hip_layout_amax_async(A.handle, C.c_void_p(ra), C.c_void_p(ca), comm.handle,
                                                 C.c_void_p(s)))


def execute_tiles_amax(src_dtype, dst_dtype, ops: np.ndarray, scalars: np.ndarray, src_base=0,
                       dst_base=0, row_scale=None, col_scale=None, row_amax=None, col_amax=None,
                       device: int = 0):
    """``execute_tiles_scaled`` plus the amax outputs: device arrays of the compute type indexed by the
    ops' target coordinates (at least one); the scales may both be None
    (costa_hip_execute_tiles_amax)."""
    sc_, dc_ = element_code(src_dtype), element_code(dst_dtype)
    ops = np.ascontiguousarray(ops, dtype=SCALED_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=_NP[_scalar_code(sc_, dc_)]).reshape(-1)
    assert sc.size % 2 == 0
    _check(lib().costa_hip_execute_tiles_amax(sc_, dc_, ops.ctypes.data_as(C.POINTER(ScaledOp)),
                                              ops.size, C.c_void_p(_ptr(src_base)),
                                              C.c_void_p(_ptr(dst_base)), sc.ctypes.data, sc.size // 2,
                                              C.c_void_p(_ptr(row_scale)), C.c_void_p(_ptr(col_scale)),
                                              C.c_void_p(_ptr(row_amax)), C.c_void_p(_ptr(col_amax)),
                                              device))


def amax_items(reset: bool = False) -> int:
    """Sub-tiles run by the amax instantiations of the scaled kernel and by the reduce-only kernel of
    ``layout_amax`` since the last reset."""
    v = C.c_int64(0)
    _check(lib().costa_hip_amax_items(C.byref(v), int(reset)))
    return v.value


# ------------------------------------------------------------------ MX block-scaled transforms
def _mx_axis(axis) -> int:
    if axis in (MX_ROWS, "rows", "ROWS"):
        return MX_ROWS
    if axis in (MX_COLS, "cols", "COLS"):
        return MX_COLS
    raise ValueError(f"axis: MX_ROWS / 'rows' or MX_COLS / 'cols', not {axis!r}")


def _mx_rounding(rounding) -> int:
    if rounding in (MX_FLOOR, "floor"):
        return MX_FLOOR
    if rounding in (MX_CEIL, "ceil"):
        return MX_CEIL
    raise ValueError(f"rounding: 'floor' or 'ceil', not {rounding!r}")


def mx_scales(tensor, axis, shape=None) -> MxScales:
    """The descriptor of a 2-D torch CUDA tensor of E8M0 bytes indexed ``[block, line]`` (``uint8``, or
    ``torch.float8_e8m0fnu`` where this torch has it); the strides are the tensor's, so
    ``torch.zeros(nb, lines)`` is block-major and ``torch.zeros(lines, nb).T`` line-major.  ``axis``:
    MX_ROWS / "rows" (a block is 32 consecutive rows of column ``line``) or MX_COLS / "cols".  With
    ``shape`` = (rows, cols) of the matrix the tensor's extent is checked too.  ValueError for a wrong
    dtype, device, rank, stride or extent.  The descriptor keeps a reference to the tensor."""
    ax = _mx_axis(axis)
    if type(tensor).__module__.split(".")[0] != "torch":
        raise ValueError(f"mx_scales: a torch CUDA tensor, not {type(tensor)}")
    if str(tensor.dtype) not in ("torch.uint8", "torch.float8_e8m0fnu"):
        raise ValueError(f"mx_scales: dtype {tensor.dtype}, scale bytes are uint8 (E8M0)")
    if not tensor.is_cuda:
        raise ValueError("mx_scales: the tensor must be device-resident (a CUDA tensor)")
    if tensor.dim() != 2:
        raise ValueError(f"mx_scales: a 2-D tensor indexed [block, line], not {tensor.dim()}-D")
    if shape is not None:
        rows, cols = shape
        along, lines = (rows, cols) if ax == MX_ROWS else (cols, rows)
        want = ((along + 31) // 32, lines)
        if tuple(tensor.shape) != want:
            raise ValueError(f"mx_scales: shape {tuple(tensor.shape)}, the matrix needs {want} "
                             "([blocks, lines])")
    bs, ls = tensor.stride()
    if (tensor.shape[0] > 1 and bs <= 0) or (tensor.shape[1] > 1 and ls <= 0):
        raise ValueError("mx_scales: the strides must be positive")
    d = MxScales(tensor.data_ptr(), ax, max(bs, 1), max(ls, 1))
    d._keep = tensor
    return d


def _mx_arg(d, what, shape=None):
    """a descriptor by reference; one made from a tensor is checked against the matrix's extent"""
    if d is None:
        return None
    if not isinstance(d, MxScales):
        raise ValueError(f"{what}: an MxScales descriptor (costa.mx_scales(tensor, axis)), not {type(d)}")
    t = getattr(d, "_keep", None)
    if t is not None and shape is not None:
        rows, cols = shape
        along, lines = (rows, cols) if d.axis == MX_ROWS else (cols, rows)
        want = ((along + 31) // 32, lines)
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: shape {tuple(t.shape)}, the {rows} x {cols} matrix needs {want} "
                             "([blocks, lines])")
    return C.byref(d)


def _sr_seed(seed):
    """a stochastic_seed argument: None, or an int in [0, 2^64)"""
    if seed is None:
        return None
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"stochastic_seed: None or an int in [0, 2^64), not {seed!r}")
    return C.c_uint64(int(seed))


def sr_bits(seed: int, i: int, j: int) -> int:
    """The 24 random bits U(seed, i, j) of target element (i, j) under stochastic rounding
    (costa_hip_sr_bits; costa_hip.h, "Stochastic rounding in the MX transforms"); host only."""
    s = _sr_seed(seed)
    if s is None:
        raise ValueError("sr_bits: seed must be an int in [0, 2^64)")
    v = C.c_uint32(0)
    _check(lib().costa_hip_sr_bits(s, int(i), int(j), C.byref(v)))
    return v.value


def transform_mx(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", alpha=1.0, beta=0.0,
                 a_scales=None, c_scales=None, rounding="floor", stream=None, stochastic_seed=None):
    """MX block-scaled transform (costa_hip_transform_mx; costa_hip.h, "MX block-scaled
    transforms"): quantise (FLOAT -> FP8, ``c_scales``), dequantise (FP8 -> FLOAT, ``a_scales``) or
    requantise (FP8 -> the same FP8, both) while redistributing, one E8M0 scale byte per 32 elements
    along the descriptor's axis.  ``a_scales`` is indexed by A's matrix as stored (before ``trans``),
    ``c_scales`` by C's; ``rounding`` is "floor" (the OCP rule, saturating) or "ceil" (no element
    saturates).  beta must be 0 with ``c_scales``.  The same three calls take packed FP4_E2M1 in
    place of FP8 (MXFP4; costa_hip.h, "MXFP4"): quantise FLOAT -> FP4_E2M1, dequantise FP4_E2M1 ->
    FLOAT, requantise FP4_E2M1 -> FP4_E2M1; no tile may split a byte (CostaError with "FP4 pair").
    And packed FP6_E2M3 / FP6_E3M2 (MXFP6; costa_hip.h, "MXFP6"): quantise FLOAT -> P, dequantise
    P -> FLOAT, requantise P -> the same P; four codes share three bytes and no tile may split such a
    group (CostaError with "FP6 quad").
    With ``stream`` the call is stream-ordered and the
    tensors must stay valid until the stream has passed it.  With several ranks each rank writes the
    ``c_scales`` bytes of its own blocks only (merge zero-initialised tensors with a MAX all-reduce)
    and needs the ``a_scales`` bytes of every block it reads.
    With ``stochastic_seed`` (an int in [0, 2^64); quantise and requantise only) the conversion rounds
    stochastically (costa_hip_transform_mx_sr; costa_hip.h, "Stochastic rounding in the MX
    transforms"): an element's decision depends on the seed, its row and column in C's matrix and its
    value alone, and the scale bytes are those of the call without a seed."""
    seed = _sr_seed(stochastic_seed)
    if not isinstance(A, Layout) or not isinstance(Cl, Layout):
        raise CostaError(1, "costa: batches of MX layout pairs are not supported")
    code = _scalar_code(A.dtype, Cl.dtype)
    ab, bb = _scalar_bytes(code, alpha), _scalar_bytes(code, beta)
    args = (A.handle, Cl.handle, _chr(trans), ab, bb, _mx_arg(a_scales, "a_scales", A.shape()),
            _mx_arg(c_scales, "c_scales", Cl.shape()), _mx_rounding(rounding))
    sr = "" if seed is None else "_sr"
    if seed is not None:
        args += (seed,)
    args += (comm.handle,)
    if stream is None:
        _check(getattr(lib(), "costa_hip_transform_mx" + sr)(*args))
    else:
        s = getattr(stream, "cuda_stream", stream) or 0
        _check(getattr(lib(), "costa_hip_transform_mx" + sr + "_async")(*args, C.c_void_p(s)))


def execute_tiles_mx(src_dtype, dst_dtype, ops: np.ndarray, scalars: np.ndarray, m: int, n: int,
                     src_base=0, dst_base=0, a_scales=None, c_scales=None, rounding="floor",
                     a_transposed: bool = False, device: int = 0, stochastic_seed=None):
    """Run a list of scaled ops (SCALED_OP_DTYPE) in one launch of the MX kernel; ``m`` x ``n`` is C's
    matrix, fp32 ``scalars``; with ``a_transposed`` A's matrix is n x m and ``a_scales`` is indexed by
    it (costa_hip_execute_tiles_mx).  With FP4_E2M1 (quantise, dequantise, requantise as for
    transform_mx) every count of an op is in elements, ``src`` / ``dst`` are byte offsets, and on each
    FP4 side the leading dimension and the extent along the stored-contiguous dimension are even.
    With FP6_E2M3 / FP6_E3M2 the same holds with multiples of 4 on each FP6 side ("FP6 quad"); a byte
    offset may have any parity.  ``stochastic_seed`` as for transform_mx
    (costa_hip_execute_tiles_mx_sr)."""
    seed = _sr_seed(stochastic_seed)
    sc_, dc_ = element_code(src_dtype), element_code(dst_dtype)
    ops = np.ascontiguousarray(ops, dtype=SCALED_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=np.float32).reshape(-1)
    assert sc.size % 2 == 0
    args = (sc_, dc_, ops.ctypes.data_as(C.POINTER(ScaledOp)), ops.size, C.c_void_p(_ptr(src_base)),
            C.c_void_p(_ptr(dst_base)), sc.ctypes.data, sc.size // 2, _mx_arg(a_scales, "a_scales"),
            _mx_arg(c_scales, "c_scales"), _mx_rounding(rounding), m, n, int(a_transposed))
    if seed is None:
        _check(lib().costa_hip_execute_tiles_mx(*args, device))
    else:
        _check(lib().costa_hip_execute_tiles_mx_sr(*args, seed, device))


def mx_items(reset: bool = False) -> int:
    """Sub-tiles run by the MX kernel since the last reset."""
    v = C.c_int64(0)
    _check(lib().costa_hip_mx_items(C.byref(v), int(reset)))
    return v.value


def mx_check_ops(ops: np.ndarray, axis, m: int, n: int):
    """The tile-boundary rule of ``c_scales`` on scaled ops (host only): CostaError with "MX block"
    when an op splits a block of C's m x n matrix along ``axis``."""
    ops = np.ascontiguousarray(ops, dtype=SCALED_OP_DTYPE)
    _check(lib().costa_hip_mx_check_ops(ops.ctypes.data_as(C.POINTER(ScaledOp)), ops.size, _mx_axis(axis),
                                        m, n))


def mx_check_scales(d: MxScales, rows: int, cols: int):
    """The stride rule of a descriptor for a rows x cols matrix (host only): positive strides, no two
    (block, line) entries on one byte."""
    _check(lib().costa_hip_mx_check_scales(C.byref(d), rows, cols))


# ------------------------------------------------------------------ dual-output MX quantise
def _seed_ref(seed):
    return None if seed is None else C.byref(seed)


def transform_mx_dual(A: Layout, Cl: Layout, Ct: Layout, comm: Comm, trans: str = "N", alpha=1.0,
                      c_scales=None, ct_scales=None, rounding="floor", stochastic_seed=None, stream=None):
    """Dual-output MX quantise (costa_hip_transform_mx_dual; costa_hip.h, "Dual-output MX quantise"):
    ``Cl`` = quantised op(A) and ``Ct`` = quantised op(A)^T, its 32-element blocks cut anew, from ONE read
    of the fp32 ``A``.  The bytes of ``Cl`` / ``c_scales`` are those of ``transform_mx(A, Cl, trans)`` and
    the bytes of ``Ct`` / ``ct_scales`` those of ``transform_mx(A, Ct)`` with the opposite ``trans``;
    ``c_scales`` is indexed by Cl's matrix, ``ct_scales`` by Ct's, each with its own axis.  Every tile of
    the (A, Cl) plan must fall, transposed, inside one block of ``Ct`` that this rank owns (CostaError
    with "dual layouts").  ``stochastic_seed`` rounds both outputs stochastically, each element keyed on
    its position in its own output.  ``stream``: stream-ordered, as for transform_mx."""
    seed = _sr_seed(stochastic_seed)
    if not all(isinstance(x, Layout) for x in (A, Cl, Ct)):
        raise CostaError(1, "costa: batches of dual MX layouts are not supported")
    ab = _scalar_bytes(FLOAT, alpha)
    args = (A.handle, Cl.handle, Ct.handle, _chr(trans), ab, _mx_arg(c_scales, "c_scales", Cl.shape()),
            _mx_arg(ct_scales, "ct_scales", Ct.shape()), _mx_rounding(rounding), _seed_ref(seed), comm.handle)
    if stream is None:
        _check(lib().costa_hip_transform_mx_dual(*args))
    else:
        s = getattr(stream, "cuda_stream", stream) or 0
        _check(lib().costa_hip_transform_mx_dual_async(*args, C.c_void_p(s)))


def execute_tiles_mx_dual(dst_dtype, ops: np.ndarray, scalars: np.ndarray, m: int, n: int, src_base=0,
                          dst_base=0, dst2_base=0, c_scales=None, ct_scales=None, rounding="floor",
                          device: int = 0, stochastic_seed=None):
    """Run a list of dual ops (DUAL_OP_DTYPE) in one launch of the dual MX kernel: FLOAT -> ``dst_dtype``
    into output 1 (``m`` x ``n``, ``c_scales``) and output 2 (``n`` x ``m``, ``ct_scales``); fp32
    ``scalars`` (costa_hip_execute_tiles_mx_dual)."""
    seed = _sr_seed(stochastic_seed)
    ops = np.ascontiguousarray(ops, dtype=DUAL_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=np.float32).reshape(-1)
    assert sc.size % 2 == 0
    _check(lib().costa_hip_execute_tiles_mx_dual(
        element_code(dst_dtype), ops.ctypes.data_as(C.POINTER(DualOp)), ops.size, C.c_void_p(_ptr(src_base)),
        C.c_void_p(_ptr(dst_base)), C.c_void_p(_ptr(dst2_base)), sc.ctypes.data, sc.size // 2,
        _mx_arg(c_scales, "c_scales"), _mx_arg(ct_scales, "ct_scales"), _mx_rounding(rounding), m, n,
        _seed_ref(seed), device))


def mx_dual_items(reset: bool = False) -> int:
    """Sub-tiles run by the dual MX kernel since the last reset (mx_items does not count them)."""
    v = C.c_int64(0)
    _check(lib().costa_hip_mx_dual_items(C.byref(v), int(reset)))
    return v.value


@dataclass
class DualPlan:
    local_dual: np.ndarray   # DUAL_OP_DTYPE: every tile that stays on the rank, with its twin in Ct
    unpack_dual: np.ndarray  # DUAL_OP_DTYPE: every tile read from the receive package, likewise
    send_elems: int = 0
    recv_elems: int = 0
    local_elems: int = 0


def plan_export_dual(A: Layout, Cl: Layout, Ct: Layout, rank: int, nranks: int, trans: str = "N", alpha=1.0,
                     c_axis=None, ct_axis=None) -> DualPlan:
    """The LOCAL and UNPACK dual ops of `rank` for transform_mx_dual (host planner, never touches a GPU),
    in the order of plan_export_scaled(A, Cl); CostaError with "dual layouts" where a tile has no twin
    in ``Ct``.  With ``c_axis`` / ``ct_axis`` the "MX block" rule of that output is checked too."""
    if not all(isinstance(x, Layout) for x in (A, Cl, Ct)):
        raise CostaError(1, "costa: batches of dual MX layouts are not supported")
    ab = _scalar_bytes(FLOAT, alpha)
    info = ScaledPlanInfo()
    ax = [-1 if a is None else _mx_axis(a) for a in (c_axis, ct_axis)]
    args = (A.handle, Cl.handle, Ct.handle, _chr(trans), ab, ax[0], ax[1], rank, nranks, C.byref(info))
    L = lib()
    _check(L.costa_hip_plan_export_dual(*args, None, None))
    ld = np.zeros(info.n_local_scaled, DUAL_OP_DTYPE)
    ud = np.zeros(info.n_unpack_scaled, DUAL_OP_DTYPE)
    _check(L.costa_hip_plan_export_dual(*args, ld.ctypes.data, ud.ctypes.data))
    b = info.base
    return DualPlan(ld, ud, b.send_elems, b.recv_elems, b.local_elems)


# ------------------------------------------------------------------ block-scaled FP8 transforms
def _block_rounding(rounding) -> int:
    if rounding in (BLOCK_EXACT, "exact"):
        return BLOCK_EXACT
    if rounding in (BLOCK_POW2, "pow2"):
        return BLOCK_POW2
    if isinstance(rounding, int):  # (an unknown value is the library's to refuse)
        return rounding
    raise ValueError(f"rounding: BLOCK_EXACT / 'exact' or BLOCK_POW2 / 'pow2', not {rounding!r}")


def _block_want(block, shape):
    rows, cols = shape
    return ((rows + block[0] - 1) // block[0], (cols + block[1] - 1) // block[1])


def block_scales(tensor, block, shape=None) -> BlockScales:
    """The descriptor of a 2-D ``float32`` torch CUDA tensor of scales indexed ``[block row, block
    column]``; the strides are the tensor's.  ``block`` is (1, 128), (128, 1) or (128, 128).  With
    ``shape`` = (rows, cols) of the matrix the tensor's extent is checked too.  ValueError for a wrong
    dtype, device, rank, block shape, stride or extent.  The descriptor keeps a reference to the
    tensor."""
    block = tuple(int(b) for b in block)
    if block not in BLOCK_SHAPES:
        raise ValueError(f"block_scales: block {block}, the shapes are (1, 128), (128, 1) and (128, 128)")
    if type(tensor).__module__.split(".")[0] != "torch":
        raise ValueError(f"block_scales: a torch CUDA tensor, not {type(tensor)}")
    if str(tensor.dtype) != "torch.float32":
        raise ValueError(f"block_scales: dtype {tensor.dtype}, the scales are float32")
    if not tensor.is_cuda:
        raise ValueError("block_scales: the tensor must be device-resident (a CUDA tensor)")
    if tensor.dim() != 2:
        raise ValueError(f"block_scales: a 2-D tensor indexed [block row, block column], not {tensor.dim()}-D")
    if shape is not None and tuple(tensor.shape) != _block_want(block, shape):
        raise ValueError(f"block_scales: shape {tuple(tensor.shape)}, the matrix needs "
                         f"{_block_want(block, shape)} ([block rows, block columns])")
    rs, cs = tensor.stride()
    if (tensor.shape[0] > 1 and rs <= 0) or (tensor.shape[1] > 1 and cs <= 0):
        raise ValueError("block_scales: the strides must be positive")
    d = BlockScales(tensor.data_ptr(), block[0], block[1], max(rs, 1), max(cs, 1))
    d._keep = tensor
    return d


def _block_arg(d, what, shape=None):
    """a descriptor by reference; one made from a tensor is checked against the matrix's extent"""
    if d is None:
        return None
    if not isinstance(d, BlockScales):
        raise ValueError(f"{what}: a BlockScales descriptor (costa.block_scales(tensor, block)), not {type(d)}")
    t = getattr(d, "_keep", None)
    if t is not None and shape is not None and (d.block_rows, d.block_cols) in BLOCK_SHAPES:
        want = _block_want((d.block_rows, d.block_cols), shape)
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: shape {tuple(t.shape)}, the {shape[0]} x {shape[1]} matrix needs {want} "
                             "([block rows, block columns])")
    return C.byref(d)


def transform_block_scaled(A: Layout, Cl: Layout, comm: Comm, trans: str = "N", alpha=1.0, beta=0.0,
                           a_scales=None, c_scales=None, rounding="exact", stream=None):
    """Block-scaled FP8 transform (costa_hip_transform_block_scaled; costa_hip.h, "Block-scaled FP8
    transforms (fp32 scales)"): quantise (FLOAT -> FP8, ``c_scales``), dequantise (FP8 -> FLOAT,
    ``a_scales``) or requantise (FP8 -> the same FP8, both; the block shapes may differ) while
    redistributing, one fp32 scale per 1 x 128, 128 x 1 or 128 x 128 block.  ``a_scales`` is indexed by
    A's matrix as stored (before ``trans``), ``c_scales`` by C's; ``rounding`` is "exact"
    (S = amax / fmax) or "pow2" (the next power of two).  beta must be 0 with ``c_scales``, and no
    tile may split a block of C (CostaError with "scale block").  With ``stream`` the call is
    stream-ordered and the tensors must stay valid until the stream has passed it.  With several ranks
    each rank writes the ``c_scales`` of its own blocks only (merge zero-initialised tensors with a
    MAX all-reduce) and needs the ``a_scales`` of every block it reads."""
    if not isinstance(A, Layout) or not isinstance(Cl, Layout):
        raise CostaError(1, "costa: batches of block-scaled layout pairs are not supported")
    code = _scalar_code(A.dtype, Cl.dtype)
    ab, bb = _scalar_bytes(code, alpha), _scalar_bytes(code, beta)
    args = (A.handle, Cl.handle, _chr(trans), ab, bb, _block_arg(a_scales, "a_scales", A.shape()),
            _block_arg(c_scales, "c_scales", Cl.shape()), _block_rounding(rounding), comm.handle)
    if stream is None:
        _check(lib().costa_hip_transform_block_scaled(*args))
    else:
        s = getattr(stream, "cuda_stream", stream) or 0
        _check(lib().costa_hip_transform_block_scaled_async(*args, C.c_void_p(s)))


def execute_tiles_block_scaled(src_dtype, dst_dtype, ops: np.ndarray, scalars: np.ndarray, m: int, n: int,
                               src_base=0, dst_base=0, a_scales=None, c_scales=None, rounding="exact",
                               a_transposed: bool = False, device: int = 0):
    """Run a list of scaled ops (SCALED_OP_DTYPE) in one launch of the block-scaled kernel; ``m`` x ``n``
    is C's matrix, fp32 ``scalars``; with ``a_transposed`` A's matrix is n x m and ``a_scales`` is
    indexed by it (costa_hip_execute_tiles_block_scaled)."""
    sc_, dc_ = element_code(src_dtype), element_code(dst_dtype)
    ops = np.ascontiguousarray(ops, dtype=SCALED_OP_DTYPE)
    sc = np.ascontiguousarray(scalars, dtype=np.float32).reshape(-1)
    assert sc.size % 2 == 0
    _check(lib().costa_hip_execute_tiles_block_scaled(
        sc_, dc_, ops.ctypes.data_as(C.POINTER(ScaledOp)), ops.size, C.c_void_p(_ptr(src_base)),
        C.c_void_p(_ptr(dst_base)), sc.ctypes.data, sc.size // 2, _block_arg(a_scales, "a_scales"),
        _block_arg(c_scales, "c_scales"), _block_rounding(rounding), m, n, int(a_transposed), device))


def block_items(reset: bool = False) -> int:
    """Work items run by the block-scaled kernels since the last reset (64 x 64 sub-tiles of
    dequantising lists, 128 x 128 regions of quantising ones)."""
    v = C.c_int64(0)
    _check(lib().costa_hip_block_items(C.byref(v), int(reset)))
    return v.value


def block_check_ops(ops: np.ndarray, block, m: int, n: int):
    """The tile-boundary rule of ``c_scales`` on scaled ops (host only): CostaError with "scale block"
    when an op splits a ``block`` = (rows, cols) block of C's m x n matrix."""
    ops = np.ascontiguousarray(ops, dtype=SCALED_OP_DTYPE)
    _check(lib().costa_hip_block_check_ops(ops.ctypes.data_as(C.POINTER(ScaledOp)), ops.size, int(block[0]),
                                           int(block[1]), m, n))


def block_check_scales(d: BlockScales, rows: int, cols: int):
    """The rules of a descriptor for a rows x cols matrix (host only): the block shape, 4-byte aligned
    data, positive strides, no two blocks on one float."""
    _check(lib().costa_hip_block_check_scales(C.byref(d), rows, cols))


@dataclass
class ScaledPlan(Plan):
    local_scaled: np.ndarray = None   # SCALED_OP_DTYPE: every tile that stays on the rank
    unpack_scaled: np.ndarray = None  # SCALED_OP_DTYPE: every tile read from the receive package


def plan_export_scaled(A: Layout, Cl: Layout, rank: int, nranks: int, trans: str = "N", alpha=1,
                       beta=0) -> ScaledPlan:
    """Tile-op lists of `rank` for a scaled transform (host planner, never touches a GPU): the
    ordinary plan with every local and unpack op in ``local_scaled`` / ``unpack_scaled``; the
    ordinary ``local_ops`` / ``unpack_ops`` are empty.  The three FP4_E2M1 pairs of transform_mx
    (quantise, dequantise, requantise) are planned too: op counts are elements, addresses bytes; when
    A holds FP4 the pack ops are byte copies and the send / receive counts are bytes.  The six pairs
    of FP6_E2M3 / FP6_E3M2 are planned the same way: a packed side's bytes are 3/4 of its elements."""
    if not isinstance(A, Layout) or not isinstance(Cl, Layout):
        raise CostaError(1, "costa: batches of scaled layout pairs are not supported")
    code = _scalar_code(A.dtype, Cl.dtype)
    ab, bb = _scalar_bytes(code, alpha), _scalar_bytes(code, beta)
    info = ScaledPlanInfo()
    L = lib()
    args = (A.handle, Cl.handle, _chr(trans), ab, bb, rank, nranks, C.byref(info))
    _check(L.costa_hip_plan_export_scaled(*args, *([None] * 8)))
    b = info.base
    po = np.zeros(b.n_pack, TILE_OP_DTYPE)
    ls = np.zeros(info.n_local_scaled, SCALED_OP_DTYPE)
    us = np.zeros(info.n_unpack_scaled, SCALED_OP_DTYPE)
    cnt = [np.zeros(nranks, np.int64) for _ in range(4)]
    sc = np.zeros(2 * b.n_slots, _NP[code])
    _check(L.costa_hip_plan_export_scaled(*args, po.ctypes.data, ls.ctypes.data, us.ctypes.data,
                                          *[x.ctypes.data for x in cnt], sc.ctypes.data))
    return ScaledPlan(np.zeros(b.n_local, TILE_OP_DTYPE), po, np.zeros(b.n_unpack, TILE_OP_DTYPE), *cnt,
                      sc, b.send_elems, b.recv_elems, b.local_elems, ls, us)


# ------------------------------------------------------------------ measurement
def set_profiling(on: bool = True):
    _check(lib().costa_hip_set_profiling(int(on)))


def get_stats(reset: bool = False) -> dict:
    s = FullStats()
    _check(lib().costa_hip_get_stats(C.byref(s), int(reset)))
    return s.as_dict()


def release_caches():
    _check(lib().costa_hip_release_caches())


def set_planner(mode: int):
    """Planner of plan-cache misses: 1 = the GPU for layout pairs of >= 4096 blocks (>= 100000
    before the first GPU plan of the process, which loads the planner's kernels; default),
    0 = always the host, 2 = the GPU wherever it applies (costa_hip_set_planner)."""
    _check(lib().costa_hip_set_planner(int(mode)))


def set_list_builder(mode: int):
    """Builder of the work lists' destination-block groups on a plan-cache miss: 1 = the GPU for
    lists of >= 16384 wavefront ops (default), 0 = always the host, 2 = the GPU wherever they apply
    (costa_hip_set_list_builder)."""
    _check(lib().costa_hip_set_list_builder(int(mode)))


@dataclass
class WorkLists:
    ordered: np.ndarray  # TILE_OP_DTYPE: [shaped ops | groups' headers and ops | wavefront pieces]
    work: np.ndarray     # uint64: sub-tile items, then the groups' header indices
    meta: dict           # the work_split counts (costa_hip_work_export)
    on_gpu: bool         # the GPU built the destination-block groups


_WORK_META = ("n_large", "n_medium", "n_skew", "n_cblock", "cblock_lds", "cb_map", "tiny_first",
              "n_tiny", "n_ordered", "n_work", "on_gpu", "flags")


def work_export(dtype, ops: np.ndarray, kind: str = "local", device=None) -> WorkLists:
    """The executor's work lists of one tile-op list (costa_hip_work_export): built on the host, or
    with ``device`` set with the destination-block groups on that GPU.  No kernel runs."""
    code = element_code(dtype)
    ops = np.ascontiguousarray(ops, dtype=TILE_OP_DTYPE)
    k = {"local": 0, "pack": 1, "unpack": 2}[kind]
    dev = -1 if device is None else int(device)
    meta = (C.c_int64 * 12)()
    L = lib()
    _check(L.costa_hip_work_export(code, ops.ctypes.data, ops.size, k, dev, None, 0, None, 0, meta))
    o = np.zeros(meta[8], TILE_OP_DTYPE)
    w = np.zeros(meta[9], np.uint64)
    _check(L.costa_hip_work_export(code, ops.ctypes.data, ops.size, k, dev, o.ctypes.data, o.size,
                                   w.ctypes.data, w.size, meta))
    m = dict(zip(_WORK_META, list(meta)))
    return WorkLists(o, w, m, bool(m["on_gpu"]))


def set_host_staging(mode: int):
    """Host-resident layouts: 1 = pipelined (default), 0 = mirror (costa_hip_set_host_staging)."""
    _check(lib().costa_hip_set_host_staging(int(mode)))


def rccl_version() -> int:
    """ncclGetVersion of the RCCL the exchange runs on in this process (major*10000 + minor*100 +
    patch): torch's bundled librccl when torch was imported first, else /opt/rocm's."""
    v = C.c_int(0)
    _check(lib().costa_hip_rccl_version(C.byref(v)))
    return v.value
