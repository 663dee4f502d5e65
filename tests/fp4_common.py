"""Shared by the MXFP4 tests (test_fp4_model_cpu.py, test_fp4_plan_cpu.py, test_gpu_fp4.py,
fp4_loopback_child.py): the numpy model of costa_hip.h, "MXFP4", built on mx_common's GLOBAL-matrix
model (gather, place, scale_g, pow2, expand, quant_data, scale_bytes).

Torch has no CPU conversion for float4_e2m1fn_x2, so the codec is numpy:
  w4(code)     the exact fp32 of a 4-bit code (bit 3 sign, bits 2..1 exponent with bias 1, bit 0
               mantissa: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6)
  cvt4(t)      finite |t| <= 6 -> code: nearest magnitude, ties to the code with mantissa bit 0, the sign
               bit of t always kept, NaN -> 0x0
  pack/unpack  two codes per byte, the element with the even index (counted from the first element of
               the buffer) in bits 3..0
A buffer of FP4 is a numpy uint8 array of PACKED bytes; the model works on its codes (one uint8 per
element, twice as long).  Every block of the test geometries starts at an even element offset of its
rank's buffer, so packing the whole buffer is packing every block.
"""
import numpy as np

import mx_common as mc
from casegen import BC, Custom
from mx_common import CEIL, COLS, F, FLOOR, ROWS  # noqa: F401

FP4 = 9
NAMES = {F: "f32", FP4: "e2m1"}
EMAX4 = 2
FMAX4 = np.float32(6.0)
MAGS = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float32)
# the seven midpoints between neighbouring magnitudes and the code each tie goes to
TIES = [(0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6)]


# ------------------------------------------------------------------ the codec
def w4(codes):
    c = np.asarray(codes, np.uint8)
    v = MAGS[c & 7]
    return np.where(c & 8, -v, v).astype(np.float32)


def cvt4(t):
    t = np.ascontiguousarray(t, np.float32)
    bits = t.view(np.uint32)
    a = np.abs(t)
    with np.errstate(invalid="ignore"):
        m = np.zeros(t.shape, np.uint8)
        for k, (mid, to) in enumerate(TIES):
            # the tie goes to the lower code k when that is the even-mantissa one, else to k + 1
            m += ((a >= np.float32(mid)) if to == k + 1 else (a > np.float32(mid))).astype(np.uint8)
    code = m | ((bits >> np.uint32(28)) & np.uint32(8)).astype(np.uint8)
    return np.where(np.isnan(t), np.uint8(0), code).astype(np.uint8)


def pack(codes):
    c = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    assert c.size % 2 == 0 and (c < 16).all()
    return (c[0::2] | (c[1::2] << 4)).astype(np.uint8)


def unpack(b):
    b = np.ascontiguousarray(b, np.uint8).reshape(-1)
    out = np.empty(b.size * 2, np.uint8)
    out[0::2] = b & 15
    out[1::2] = b >> 4
    return out


def widen(buf, code):
    """a buffer of `code` -> fp32 per element"""
    return np.ascontiguousarray(buf, np.float32).copy() if code == F else w4(unpack(buf))


def narrow(x, code):
    """fp32 per element -> a buffer of `code` (exact for values that are w4 of a code)"""
    return np.ascontiguousarray(x, np.float32).copy() if code == F else pack(cvt4(x))


def buf_bytes(code, n_elems):
    return n_elems * 4 if code == F else n_elems // 2


def fp4_data(seed, n):
    """n elements of random codes (all 16, -0 included), packed"""
    return pack(np.random.default_rng(seed).integers(0, 16, n).astype(np.uint8))


def fill(code, seed, n):
    """the old contents of a destination of n elements"""
    if code == F:
        return mc.fc.gen(F, seed, n)
    return fp4_data(seed, n)


# ------------------------------------------------------------------ the block rule
def quantise_dense4(V, axis, rounding=FLOOR):
    """(codes m x n uint8, E bytes [block, line], t = the scaled values before the clamp): mx_common's
    quantise_dense with emax = 2, fmax = 6 and cvt4; a block with E = 255 stores code 0x0 everywhere"""
    V = np.ascontiguousarray(V, np.float32)
    W = V if axis == ROWS else V.T
    along, lines = W.shape
    nb = mc.n_blocks(along)
    pad = np.zeros((nb * 32, lines), np.float32)
    pad[:along] = W
    bits = pad.view(np.uint32) & np.uint32(0x7FFFFFFF)
    amax = bits.reshape(nb, 32, lines).max(axis=1)
    e = (amax >> np.uint32(23)).astype(np.int64)
    E = np.where(e == 255, 255, np.clip(e - EMAX4, 0, 254))
    with np.errstate(all="ignore"):
        if rounding == CEIL:
            over = amax.view(np.float32) * mc.pow2(np.where(E == 255, 0, 254 - E)) > FMAX4
            E = np.where((E != 255) & over & (E < 254), E + 1, E)
        inv = mc.pow2(np.where(E == 255, 255, 254 - E))
        t = pad * np.repeat(inv, 32, axis=0)
        assert t.dtype == np.float32
    t = np.where(np.repeat(E == 255, 32, axis=0), np.float32(np.nan), t)[:along]
    with np.errstate(invalid="ignore"):
        q = cvt4(np.clip(t, -FMAX4, FMAX4))
    if axis == COLS:
        q, t = q.T, t.T
    return np.ascontiguousarray(q), E.astype(np.uint8), np.ascontiguousarray(t)


# ------------------------------------------------------------------ layouts
def make_layout(costa, case, rank, ptr, P, code):
    """the product's layout of `case` over a buffer of `code` at BYTE address `ptr`: every count in
    elements, element offsets turned into byte pointers (off / 2 for FP4)"""
    if code != FP4:
        return mc.make_layout(costa, case, rank, ptr, P, code)
    if isinstance(case, BC):
        return case.make_layout(rank, ptr, P, code)
    per, _ = case._blocks(P)
    assert all(off % 2 == 0 and ld % 2 == 0 for _, _, off, ld in per[rank])
    blocks = [(ptr + off // 2, ld, i, j) for i, j, off, ld in per[rank]]
    nbr, nbc = case.owners.shape
    return costa.custom_layout(nbr, nbc, case.rowsplit, case.colsplit, case.owners, blocks, case.ord, code)


def geometry(name, op, grid=(1, 1)):
    """(A case, C case) of the MXFP4 tests: 202 x 158 (both = 2 mod 4: 6 * 32 + 10 and 4 * 32 + 30),
    split points on multiples of 32, even lld / ld paddings and gaps"""
    t = op != "N"
    pm, pn = grid
    P = pm * pn
    kw = dict(pm=pm, pn=pn)

    def dims(m, n):
        return (n, m) if t else (m, n)
    if name == "g202":
        return BC(*dims(202, 158), 64, 96, **kw), BC(202, 158, 96, 32, **kw)
    if name == "g202pad":
        return BC(*dims(202, 158), 64, 96, lld_pad=2, **kw), BC(202, 158, 96, 32, lld_pad=2, **kw)
    if name == "custom32":
        rs, cs = [0, 64, 96, 200], [0, 32, 128, 170]
        ars, acs = [0, 96, 200], [0, 64, 170]
        if t:
            ars, acs = acs, ars

        def owners(nr, nc, k):
            i, j = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
            return ((i * k + j) % P).astype(np.int32)
        return (Custom(ars, acs, owners(len(ars) - 1, len(acs) - 1, 1), ord="R", ld_pad=2, gap=4),
                Custom(rs, cs, owners(len(rs) - 1, len(cs) - 1, 3), ord="C", ld_pad=2, gap=6))
    raise KeyError(name)


# ------------------------------------------------------------------ expected values
def expected_transform_mx4(ta, tc, op, alpha, beta, a_case, c_case, P, a_bufs, c_bufs, sa=None, a_axis=ROWS,
                           c_axis=None, rounding=FLOOR):
    """-> (expected C buffer of every rank in tc, SC[block, line] or None, t before the clamp or None);
    mx_common.expected_transform_mx with the FP4 codec"""
    am, an = a_case.shape()
    X = mc.gather(a_case, P, [widen(a, ta) for a in a_bufs])
    if sa is not None:
        with np.errstate(all="ignore"):
            X = X * mc.expand(sa, a_axis, am, an)
    if op != "N":
        X = X.T
    wc = [widen(c, tc) for c in c_bufs]
    V = mc.scale_g(np.ascontiguousarray(X, np.float32), mc.gather(c_case, P, wc) if beta != 0 else None, alpha, beta)
    assert V.dtype == np.float32 and V.shape == tuple(c_case.shape())
    if c_axis is None:
        assert tc == F
        return mc.place(c_case, P, V, wc), None, None
    q, E, t = quantise_dense4(V, c_axis, rounding)
    out = mc.place(c_case, P, w4(q), wc)
    return [narrow(o, tc) for o in out], E, t


def expected_tiles_mx4(ta, tc, sops, alpha, beta, a, c, m, n, sa=None, a_axis=ROWS, a_transposed=False,
                       c_axis=None, rounding=FLOOR, sc_fill=None):
    """mx_common.expected_tiles_mx with the FP4 codec; the ops' src / dst count ELEMENTS.
    -> (expected destination buffer in tc, expected c_scales over sc_fill, t on the covered elements)"""
    wa, wc = widen(a, ta), widen(c, tc)
    V = np.zeros((m, n), np.float32)
    cov = np.zeros((m, n), bool)
    fac = None
    if sa is not None:
        fac = mc.expand(sa, a_axis, n, m).T if a_transposed else mc.expand(sa, a_axis, m, n)
    for t in sops:
        si, di, i, j = mc.op_index(t)
        assert not cov[i, j].any(), "ops overlap in target coordinates"
        cov[i, j] = True
        x = wa[si]
        with np.errstate(all="ignore"):
            if fac is not None:
                x = x * fac[i, j]
        V[i, j] = mc.scale_g(x.astype(np.float32), wc[di], alpha, beta)
    if c_axis is None:
        out = wc.copy()
        for t in sops:
            si, di, i, j = mc.op_index(t)
            out[di] = V[i, j]
        return out, None, None
    q, E, tt = quantise_dense4(V, c_axis, rounding)
    oc = unpack(c)
    for t in sops:
        si, di, i, j = mc.op_index(t)
        oc[di] = q[i, j]
    Wc = cov if c_axis == ROWS else cov.T
    first = Wc[::32, :]
    sc = np.asarray(sc_fill, np.uint8).copy()
    assert sc.shape == E.shape
    sc[first] = E[first]
    return pack(oc), sc, np.where(cov, tt, 0)


def assert_same(got, exp, code, what):
    """every bit of the whole buffer (FP4 has no NaN; an expected fp32 NaN only asks for a NaN)"""
    if code == F:
        return mc.assert_bits(got, exp, F, what)
    g, e = np.ascontiguousarray(got, np.uint8).reshape(-1), np.ascontiguousarray(exp, np.uint8).reshape(-1)
    assert g.size == e.size, f"{what}: {g.size} bytes, {e.size} expected"
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} bytes differ, first at byte {bad[0]}: "
                           f"got {int(g[bad[0]]):#04x}, expected {int(e[bad[0]]):#04x}")


# ------------------------------------------------------------------ the evenness rule on exported ops
def op_even(t, ta, tc):
    """the per-op half of the rule on one exported scaled op"""
    o = t["op"]
    nf, ns, lds, ldd, tr = int(o["nf"]), int(o["ns"]), int(o["lds"]), int(o["ldd"]), bool(int(o["flags"]) & 1)
    ok = True
    if ta == FP4:
        ok = ok and nf % 2 == 0 and lds % 2 == 0
    if tc == FP4:
        ok = ok and (ns if tr else nf) % 2 == 0 and ldd % 2 == 0
    return ok
