"""Shared by the half-precision tests (test_half_plan_cpu.py, test_gpu_half.py,
half_loopback_child.py): the element-type codes, the geometries of tests/test_gpu_mixed.py, layouts
of a 2-byte type (casegen.ESIZE does not know the new codes, so custom-layout block addresses are
computed here from Custom._blocks), and the expected values.

Expected values always come from the CPU oracle run in FLOAT: with w() the exact widening to fp32
and cvt() the rounding fp32 -> H (numpy astype(float16); torch-CPU .to(bfloat16)),
    H -> H       cvt(oracle(FLOAT, w(a), w(c)))
    FLOAT -> H   the same on w(cvt(a))
    H -> FLOAT   oracle(FLOAT, w(a), c)
Buffers of a 2-byte type are numpy uint16 arrays of raw bits.
"""
import numpy as np

import oracle
from casegen import BC, Custom

F, H16, BF16 = 0, 5, 6
NAMES = {F: "f32", H16: "f16", BF16: "bf16"}
CNAMES = {0: "FLOAT", 1: "DOUBLE", 2: "CFLOAT", 3: "CDOUBLE", 4: "INT32", 5: "HALF", 6: "BFLOAT16"}
ESIZE = {0: 4, 1: 8, 2: 8, 3: 16, 4: 4, 5: 2, 6: 2}
# the supported pairs
PAIRS = [(H16, H16), (BF16, BF16), (F, H16), (F, BF16), (H16, F), (BF16, F)]
PAIR_IDS = [f"{NAMES[a]}-{NAMES[c]}" for a, c in PAIRS]


# ------------------------------------------------------------------ conversions
def cvt(x, code):
    """fp32 array -> elements of `code`: raw uint16 bits for the 2-byte types"""
    x = np.ascontiguousarray(x, np.float32)
    if code == F:
        return x.copy()
    if code == H16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    import torch
    return torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def widen(b, code):
    """elements of `code` -> fp32, exactly"""
    if code == F:
        return np.ascontiguousarray(b, np.float32).copy()
    b = np.ascontiguousarray(b, np.uint16)
    if code == H16:
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def gen(code, seed, n):
    """n elements of `code` from the oracle's FLOAT stream (values in +-(2e-5 .. 1))"""
    return cvt(oracle.gen(oracle.FLOAT, seed, 0, n), code)


def assert_bits(got, exp, code, what):
    """raw bits over the whole buffer, except that an expected NaN only asks for a NaN"""
    ut = np.uint32 if code == F else np.uint16
    g, e = np.ascontiguousarray(got).view(ut).reshape(-1), np.ascontiguousarray(exp).view(ut).reshape(-1)
    assert g.size == e.size, f"{what}: {g.size} elements, {e.size} expected"
    nan = np.isnan(widen(e.view(np.float32) if code == F else e, code))
    assert np.isnan(widen(g.view(np.float32) if code == F else g, code)[nan]).all(), f"{what}: NaN expected"
    bad = np.flatnonzero((g != e) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} elements differ, first at {bad[0]}: "
                           f"got {int(g[bad[0]]):#x}, expected {int(e[bad[0]]):#x}")


# ------------------------------------------------------------------ geometries (test_gpu_mixed.py)
def _cfg5_small(op, P):
    from cases import _edges
    m, n = 2048, 1920
    am, an = (n, m) if op != "N" else (m, n)
    ars, acs = _edges(0xC5A1, am, 8, 96), _edges(0xC5A2, an, 8, 96)
    crs, ccs = _edges(0xC5A3, m, 16, 160), _edges(0xC5A4, n, 16, 160)

    def owners(nr, nc, k):
        i, j = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
        return ((i * k + j) % P).astype(np.int32)
    return (Custom(ars, acs, owners(len(ars) - 1, len(acs) - 1, 1)),
            Custom(crs, ccs, owners(len(crs) - 1, len(ccs) - 1, 3)))


def geometry(name, op, grid=(1, 1)):
    """(A case, C case) of a geometry of tests/test_gpu_mixed.py on a pm x pn rank grid"""
    t = op != "N"
    pm, pn = grid
    kw = dict(pm=pm, pn=pn)

    def dims(m, n):
        return (n, m) if t else (m, n)
    if name == "bc203":
        return BC(*dims(203, 157), 32, 48, **kw), BC(203, 157, 40, 24, **kw)
    if name == "whole":
        return BC(256, 256, 128, 128, **kw), BC(256, 256, 128, 128, **kw)
    if name == "oneblock":
        am, an = dims(300, 260)
        return BC(am, an, am, an, **kw), BC(300, 260, 64, 64, **kw)
    if name == "cfg5":
        return _cfg5_small(op, pm * pn)
    if name == "lldpad":
        return BC(*dims(203, 157), 32, 48, lld_pad=1, **kw), BC(203, 157, 40, 24, lld_pad=1, **kw)
    raise KeyError(name)


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
    wa = widen(cvt(widen(a, ta), tc) if ta == F else a, tc if ta == F else ta)
    wc = widen(c, tc)
    oracle.transform(oracle.FLOAT, op, alpha, beta, a_case.geom(1), [wa], c_case.geom(1), [wc])
    return cvt(wc, tc)


def expected_tiles(ta, tc, ops, scal, a, c):
    """the whole expected destination buffer of a tile-op list; `ops` address elements (src and dst
    offsets in elements)"""
    wa = widen(cvt(widen(a, ta), tc) if ta == F else a, tc if ta == F else ta)
    wc = widen(c, tc)
    o = ops.copy()
    o["src"] = ops["src"] * 4
    o["dst"] = ops["dst"] * 4
    oracle.exec_tile_ops(oracle.FLOAT, o, np.asarray(scal, np.float32), wa.ctypes.data, wc.ctypes.data)
    return cvt(wc, tc)
