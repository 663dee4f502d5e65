"""Shared by the dual-output MX tests (test_mx_dual_plan_cpu.py, test_gpu_mx_dual.py,
mx_dual_loopback_child.py): the transposed twin of a target layout, the geometries per type and the
expected bytes of costa_hip.h, "Dual-output MX quantise" -- the CPU models the MX tests already have
(mx_common, fp4_common, fp6_common, mx_sr_common), applied twice: once to op(A) for C, once to op(A)^T for
Ct."""
import numpy as np

import fp4_common as f4
import fp6_common as f6
import mx_common as mc
import mx_sr_common as sr
from casegen import BC, Custom
from mx_sr_common import E2M3, E3M2, E4M3, E5M2, F, FP4, NAMES, QTYPES  # noqa: F401

TR, F_ROWS, VEC_DST = 0x1, 0x80, 0x8
OTHER = {"N": "T", "T": "N", "C": "N"}
# (type, geometry) pairs of the issue: mx_common's four for FP8, fp4_common's and fp6_common's two each
GEOMS = [(E4M3, "g192"), (E5M2, "g203"), (E4M3, "g203pad"), (E5M2, "custom32"), (FP4, "g202"), (FP4, "custom32"),
         (E2M3, "g204"), (E3M2, "custom32q")]
GEOM_IDS = [f"{NAMES[t]}-{g}" for t, g in GEOMS]


def geometry(tq, name, op, grid=(1, 1)):
    if tq == FP4:
        return f4.geometry(name, op, grid)
    if tq in f6.FP6:
        return f6.geometry(name, op, grid)
    return mc.geometry(name, op, grid)


def twin(c_case, ord_):
    """the transposed twin of a target layout, stored in ordering `ord_`: transposed split points with
    transposed owners (block-cyclic: the process grid turned round, its rank order flipped)"""
    if isinstance(c_case, BC):
        assert c_case.ia == 1 and c_case.ja == 1 and c_case.rsrc == 0 and c_case.csrc == 0
        return BC(c_case.n, c_case.m, c_case.nb, c_case.mb, pm=c_case.pn, pn=c_case.pm,
                  order="C" if c_case.order.upper() == "R" else "R", ord=ord_, lld_pad=c_case.lld_pad)
    pad = c_case.ld_pad
    return Custom(list(c_case.colsplit), list(c_case.rowsplit), c_case.owners.T.copy(), ord=ord_, ld_pad=pad,
                  gap=c_case.gap)


def sc_shape(m, n, axis):
    return (mc.n_blocks(m), n) if axis == mc.ROWS else (mc.n_blocks(n), m)


def twin_ops(dops):
    """output 2's side of dual ops (ELEMENT offsets) as scaled ops of its own n x m matrix"""
    import costa_amd
    t = np.zeros(len(dops), costa_amd.SCALED_OP_DTYPE)
    t["op"] = dops["s"]["op"]
    t["op"]["dst"] = dops["dst2"]
    t["op"]["ldd"] = dops["ldd2"]
    t["op"]["flags"] = ((dops["s"]["op"]["flags"] & ~np.uint32(TR | VEC_DST)) ^ np.uint32(F_ROWS)) | \
        (dops["flags2"] & np.uint32(TR))
    t["row0"] = dops["s"]["col0"]
    t["col0"] = dops["s"]["row0"]
    return t


def expected_tiles(tq, dops, alpha, src, dst0, dst20, m, n, c_axis, ct_axis, rounding, sc0, sct0, seed=None):
    """-> ((C buffer, c_scales, t before the clamp), (Ct buffer, ct_scales, t)) of a dual tile list whose
    offsets count ELEMENTS; with `seed` the SR bytes (Ct keyed on its own (row, column) = (j, i))"""
    out = []
    for ops, dst, mm, nn, axis, fill in ((dops["s"], dst0, m, n, c_axis, sc0), (twin_ops(dops), dst20, n, m, ct_axis, sct0)):
        if seed is None:
            out.append(sr.family(tq)[1](F, tq, ops, alpha, 0.0, src, dst, mm, nn, c_axis=axis, rounding=rounding,
                                        sc_fill=fill))
        else:
            r = sr.expected_tiles_mx_sr(seed, F, tq, ops, alpha, 0.0, src, dst, mm, nn, c_axis=axis, rounding=rounding,
                                        sc_fill=fill)
            out.append((r.exp, r.sc, r.t_pre))
    return out


def expected_transform(tq, op, alpha, a_case, c_case, ct_case, P, a, c, ct, c_axis, ct_axis, rounding, seed=None):
    """-> ((C buffers per rank, SC, t), (Ct buffers per rank, SCt, t))"""
    out = []
    for o, case, bufs, axis in ((op, c_case, c, c_axis), (OTHER[op], ct_case, ct, ct_axis)):
        if seed is None:
            out.append(sr.family(tq)[0](F, tq, o, alpha, 0.0, a_case, case, P, a, bufs, c_axis=axis, rounding=rounding))
        else:
            r = sr.expected_transform_mx_sr(seed, F, tq, o, alpha, 0.0, a_case, case, P, a, bufs, c_axis=axis,
                                            rounding=rounding)
            out.append((r.exp, r.sc, r.t_pre))
    return out


def assert_finite(bufs, tq, what):
    for b in (bufs if isinstance(bufs, list) else [bufs]):
        sr.assert_finite(b, tq, what)
