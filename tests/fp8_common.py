"""Shared by the FP8 tests (test_fp8_plan_cpu.py, test_gpu_fp8.py, fp8_loopback_child.py): the
element-type codes, layouts of a 1-byte type over the geometries of half_common.geometry, and the
expected values.

Expected values always come from the CPU oracle run in FLOAT on widened inputs, with cvt applied
once: with w() the exact widening to fp32 (torch-CPU .to(float32)) and cvt() the conversion
fp32 -> Q (torch-CPU .to(float8 dtype)),
    Q -> Q       cvt(oracle(FLOAT, w(a), w(c)))
    FLOAT -> Q   cvt(oracle(FLOAT, a, w(c)))       the oracle reads A unrounded
    Q -> FLOAT   oracle(FLOAT, w(a), c)
Buffers of a 1-byte type are numpy uint8 arrays of raw bits.
"""
import numpy as np

import oracle
from casegen import BC
from half_common import geometry  # noqa: F401  (re-exported)

F, E4M3, E5M2 = 0, 7, 8
NAMES = {F: "f32", E4M3: "e4m3", E5M2: "e5m2"}
CNAMES = {0: "FLOAT", 1: "DOUBLE", 2: "CFLOAT", 3: "CDOUBLE", 4: "INT32", 5: "HALF", 6: "BFLOAT16",
          7: "FP8_E4M3", 8: "FP8_E5M2"}
ESIZE = {0: 4, 1: 8, 2: 8, 3: 16, 4: 4, 5: 2, 6: 2, 7: 1, 8: 1}
# the supported pairs
PAIRS = [(E4M3, E4M3), (E5M2, E5M2), (F, E4M3), (F, E5M2), (E4M3, F), (E5M2, F)]
PAIR_IDS = [f"{NAMES[a]}-{NAMES[c]}" for a, c in PAIRS]


def pkg_code(ta, tc):
    """the element type of the exchange's packages: A's"""
    return ta


def _torch_dt(code):
    import torch
    return {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}[code]


# ------------------------------------------------------------------ conversions
def cvt(x, code):
    """fp32 array -> elements of `code`: raw uint8 bits for the 1-byte types"""
    x = np.ascontiguousarray(x, np.float32)
    if code == F:
        return x.copy()
    import torch
    return torch.from_numpy(x.copy()).to(_torch_dt(code)).view(torch.uint8).numpy().copy()


def widen(b, code):
    """elements of `code` -> fp32, exactly"""
    if code == F:
        return np.ascontiguousarray(b, np.float32).copy()
    import torch
    b = np.ascontiguousarray(b, np.uint8)
    return torch.from_numpy(b.copy()).view(_torch_dt(code)).to(torch.float32).numpy().copy()


def gen(code, seed, n):
    """n elements of `code` from the oracle's FLOAT stream (values in +-(2e-5 .. 1))"""
    return cvt(oracle.gen(oracle.FLOAT, seed, 0, n), code)


def assert_bits(got, exp, code, what):
    """raw bits over the whole buffer, except that an expected NaN only asks for a NaN"""
    ut = np.uint32 if code == F else np.uint8
    g, e = np.ascontiguousarray(got).view(ut).reshape(-1), np.ascontiguousarray(exp).view(ut).reshape(-1)
    assert g.size == e.size, f"{what}: {g.size} elements, {e.size} expected"
    nan = np.isnan(widen(e.view(np.float32) if code == F else e, code))
    assert np.isnan(widen(g.view(np.float32) if code == F else g, code)[nan]).all(), f"{what}: NaN expected"
    bad = np.flatnonzero((g != e) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} elements differ, first at {bad[0]}: "
                           f"got {int(g[bad[0]]):#x}, expected {int(e[bad[0]]):#x}")


# ------------------------------------------------------------------ layouts
def make_layout(costa, case, rank, ptr, P, code):
    """the product's layout of `case` over a buffer of `code` at address `ptr`"""
    if isinstance(case, BC):
        return case.make_layout(rank, ptr, P, code)  # (passes the code through)
    per, _ = case._blocks(P)
    E = ESIZE[code]
    blocks = [(ptr + off * E, ld, i, j) for i, j, off, ld in per[rank]]
    nbr, nbc = case.owners.shape
    return costa.custom_layout(nbr, nbc, case.rowsplit, case.colsplit, case.owners, blocks, case.ord, code)


# ------------------------------------------------------------------ expected values
def expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c):
    """the whole expected C buffer (elements of tc) of a one-rank transform"""
    wa, wc = widen(a, ta), widen(c, tc)
    oracle.transform(oracle.FLOAT, op, alpha, beta, a_case.geom(1), [wa], c_case.geom(1), [wc])
    return cvt(wc, tc)


def expected_tiles(ta, tc, ops, scal, a, c):
    """the whole expected destination buffer of a tile-op list; `ops` address elements (src and dst
    offsets in elements).  Scale kind BITCOPY of the oracle is a copy of the fp32 value, and cvt of
    a widened Q value gives its bits back for every non-NaN input."""
    wa, wc = widen(a, ta), widen(c, tc)
    o = ops.copy()
    o["src"] = ops["src"] * 4
    o["dst"] = ops["dst"] * 4
    oracle.exec_tile_ops(oracle.FLOAT, o, np.asarray(scal, np.float32), wa.ctypes.data, wc.ctypes.data)
    return cvt(wc, tc)
