"""Shared by the MXFP6 tests (test_fp6_model_cpu.py, test_fp6_plan_cpu.py, test_gpu_fp6.py,
fp6_loopback_child.py): the numpy model of costa_hip.h, "MXFP6", built on mx_common's GLOBAL-matrix
model (gather, place, scale_g, pow2, expand, quant_data, scale_bytes).

Neither numpy nor torch has an FP6 type, so the codec is numpy and table-based, independent of the
kernel's integer rounding:
  w6(code, P)   the exact fp32 of a 6-bit code (bit 5 the sign) from the 32-entry magnitude table of P
  cvt6(t, P)    finite |t| <= fmax -> code: comparisons against the 31 midpoints of neighbouring
                magnitudes, each with an explicit tie target (the code whose mantissa is even); the
                sign bit of t always kept, NaN -> 0x00
  pack/unpack   four codes per three bytes, w = c0 | c1 << 6 | c2 << 12 | c3 << 18, bytes low to high;
                elements counted from the first element of the buffer
A buffer of FP6 is a numpy uint8 array of PACKED bytes; the model works on its codes (one uint8 per
element, 4/3 as long).  Every block of the test geometries starts at a multiple of 4 elements of its
rank's buffer, so packing the whole buffer is packing every block.
"""
import numpy as np

import mx_common as mc
from casegen import BC, Custom
from mx_common import CEIL, COLS, F, FLOOR, ROWS  # noqa: F401

E2M3, E3M2 = 10, 11
FP6 = (E2M3, E3M2)
FP4, E4M3 = 9, 7
NAMES = {F: "f32", E2M3: "e2m3", E3M2: "e3m2"}
TYPE_NAMES = {E2M3: "FP6_E2M3", E3M2: "FP6_E3M2"}
EMAX = {E2M3: 2, E3M2: 4}
FMAX = {E2M3: np.float32(7.5), E3M2: np.float32(28.0)}
FMAX_BITS = {E2M3: 0x40F00000, E3M2: 0x41E00000}
MIN_NORMAL = {E2M3: np.float32(1.0), E3M2: np.float32(0.25)}
MIN_SUBNORMAL = {E2M3: np.float32(0.125), E3M2: np.float32(0.0625)}


def _mags(mb, bias):
    out = []
    for c in range(32):
        e, m = c >> mb, c & ((1 << mb) - 1)
        out.append(m / (1 << mb) * 2.0 ** (1 - bias) if e == 0 else (1 + m / (1 << mb)) * 2.0 ** (e - bias))
    return np.array(out, np.float32)


# the magnitudes of codes 0 .. 31 (written out for e2m3's first and last rows as a check of _mags)
MAGS = {E2M3: _mags(3, 1), E3M2: _mags(2, 3)}
assert list(MAGS[E2M3][:9]) == [0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0] and MAGS[E2M3][31] == 7.5
assert list(MAGS[E3M2][:5]) == [0, 0.0625, 0.125, 0.1875, 0.25] and MAGS[E3M2][31] == 28.0
for _p in FP6:
    assert (np.diff(MAGS[_p]) > 0).all() and MAGS[_p][31] == FMAX[_p]
    assert MAGS[_p].view(np.uint32)[31] == FMAX_BITS[_p]
# the 31 midpoints between neighbouring magnitudes (exact in fp32) and the code each tie goes to: of
# codes k and k + 1 the one whose mantissa (hence whose code) is even
TIES = {p: [(np.float32((float(MAGS[p][k]) + float(MAGS[p][k + 1])) / 2), k if k % 2 == 0 else k + 1)
            for k in range(31)] for p in FP6}
for _p in FP6:
    for _k, (_mid, _) in enumerate(TIES[_p]):
        assert float(_mid) * 2 == float(MAGS[_p][_k]) + float(MAGS[_p][_k + 1])


# ------------------------------------------------------------------ the codec
def w6(codes, p):
    c = np.asarray(codes, np.uint8)
    v = MAGS[p][c & 31]
    return np.where(c & 32, -v, v).astype(np.float32)


def cvt6(t, p):
    t = np.ascontiguousarray(t, np.float32)
    bits = t.view(np.uint32)
    a = np.abs(t)
    with np.errstate(invalid="ignore"):
        m = np.zeros(t.shape, np.uint8)
        for k, (mid, to) in enumerate(TIES[p]):
            # the tie stays at the lower code k when that is the even one, else it goes up to k + 1
            m += ((a >= mid) if to == k + 1 else (a > mid)).astype(np.uint8)
    code = m | ((bits >> np.uint32(26)) & np.uint32(32)).astype(np.uint8)
    return np.where(np.isnan(t), np.uint8(0), code).astype(np.uint8)


def pack(codes):
    c = np.ascontiguousarray(codes, np.uint8).reshape(-1).astype(np.uint32)
    assert c.size % 4 == 0 and (c < 64).all()
    w = c[0::4] | (c[1::4] << 6) | (c[2::4] << 12) | (c[3::4] << 18)
    out = np.empty(c.size // 4 * 3, np.uint8)
    out[0::3] = w & 0xFF
    out[1::3] = (w >> 8) & 0xFF
    out[2::3] = w >> 16
    return out


def unpack(b):
    b = np.ascontiguousarray(b, np.uint8).reshape(-1).astype(np.uint32)
    assert b.size % 3 == 0
    w = b[0::3] | (b[1::3] << 8) | (b[2::3] << 16)
    out = np.empty(b.size // 3 * 4, np.uint8)
    for k in range(4):
        out[k::4] = (w >> (6 * k)) & 63
    return out


def widen(buf, code):
    """a buffer of `code` -> fp32 per element"""
    return np.ascontiguousarray(buf, np.float32).copy() if code == F else w6(unpack(buf), code)


def narrow(x, code):
    """fp32 per element -> a buffer of `code` (exact for values that are w6 of a code)"""
    return np.ascontiguousarray(x, np.float32).copy() if code == F else pack(cvt6(x, code))


def buf_bytes(code, n_elems):
    return n_elems * 4 if code == F else n_elems * 3 // 4


def addr(code, off):
    """byte offset of element offset `off` in a buffer of `code`"""
    if code == F:
        return off * 4
    assert off % 4 == 0
    return off * 3 // 4


def fp6_data(seed, n):
    """n elements of random codes (all 64, -0 included), packed"""
    return pack(np.random.default_rng(seed).integers(0, 64, n).astype(np.uint8))


def fill(code, seed, n):
    """the old contents of a destination of n elements"""
    if code == F:
        return mc.fc.gen(F, seed, n)
    return fp6_data(seed, n)


# ------------------------------------------------------------------ the block rule
def quantise_dense6(V, axis, p, rounding=FLOOR):
    """(codes m x n uint8, E bytes [block, line], t = the scaled values before the clamp): mx_common's
    quantise_dense with the emax / fmax of p and cvt6; a block with E = 255 stores code 0x00 everywhere"""
    V = np.ascontiguousarray(V, np.float32)
    W = V if axis == ROWS else V.T
    along, lines = W.shape
    nb = mc.n_blocks(along)
    pad = np.zeros((nb * 32, lines), np.float32)
    pad[:along] = W
    bits = pad.view(np.uint32) & np.uint32(0x7FFFFFFF)
    amax = bits.reshape(nb, 32, lines).max(axis=1)
    e = (amax >> np.uint32(23)).astype(np.int64)
    E = np.where(e == 255, 255, np.clip(e - EMAX[p], 0, 254))
    with np.errstate(all="ignore"):
        if rounding == CEIL:
            over = amax.view(np.float32) * mc.pow2(np.where(E == 255, 0, 254 - E)) > FMAX[p]
            E = np.where((E != 255) & over & (E < 254), E + 1, E)
        inv = mc.pow2(np.where(E == 255, 255, 254 - E))
        t = pad * np.repeat(inv, 32, axis=0)
        assert t.dtype == np.float32
    t = np.where(np.repeat(E == 255, 32, axis=0), np.float32(np.nan), t)[:along]
    with np.errstate(invalid="ignore"):
        q = cvt6(np.clip(t, -FMAX[p], FMAX[p]), p)
    if axis == COLS:
        q, t = q.T, t.T
    return np.ascontiguousarray(q), E.astype(np.uint8), np.ascontiguousarray(t)


# ------------------------------------------------------------------ layouts
def make_layout(costa, case, rank, ptr, P, code):
    """the product's layout of `case` over a buffer of `code` at BYTE address `ptr`: every count in
    elements, element offsets turned into byte pointers (off * 3 / 4 for FP6)"""
    if code not in FP6:
        return mc.make_layout(costa, case, rank, ptr, P, code)
    if isinstance(case, BC):
        return case.make_layout(rank, ptr, P, code)
    per, _ = case._blocks(P)
    assert all(off % 4 == 0 and ld % 4 == 0 for _, _, off, ld in per[rank])
    blocks = [(ptr + off * 3 // 4, ld, i, j) for i, j, off, ld in per[rank]]
    nbr, nbc = case.owners.shape
    return costa.custom_layout(nbr, nbc, case.rowsplit, case.colsplit, case.owners, blocks, case.ord, code)


GEOMETRIES = ("g204", "g204pad", "custom32q")


def geometry(name, op, grid=(1, 1)):
    """(A case, C case) of the MXFP6 tests: 204 x 156 (6 * 32 + 12 by 4 * 32 + 28), split points on
    multiples of 32, lld / ld paddings and gaps that are multiples of 4 elements.  g204 on one rank has
    lld 204 = 4 mod 8: a byte pitch of 153, odd; custom32q's gaps of 4 and 12 elements are 3 and 9
    bytes, so blocks sit at odd byte addresses"""
    t = op != "N"
    pm, pn = grid
    P = pm * pn
    kw = dict(pm=pm, pn=pn)

    def dims(m, n):
        return (n, m) if t else (m, n)
    if name == "g204":
        return BC(*dims(204, 156), 64, 96, **kw), BC(204, 156, 96, 32, **kw)
    if name == "g204pad":
        return BC(*dims(204, 156), 64, 96, lld_pad=4, **kw), BC(204, 156, 96, 32, lld_pad=4, **kw)
    if name == "custom32q":
        rs, cs = [0, 64, 96, 200], [0, 32, 128, 172]
        ars, acs = [0, 96, 200], [0, 64, 172]
        if t:
            ars, acs = acs, ars

        def owners(nr, nc, k):
            i, j = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
            return ((i * k + j) % P).astype(np.int32)
        return (Custom(ars, acs, owners(len(ars) - 1, len(acs) - 1, 1), ord="R", ld_pad=4, gap=4),
                Custom(rs, cs, owners(len(rs) - 1, len(cs) - 1, 3), ord="C", ld_pad=4, gap=12))
    raise KeyError(name)


# ------------------------------------------------------------------ expected values
def _p_of(ta, tc):
    return tc if tc in FP6 else ta


def expected_transform_mx6(ta, tc, op, alpha, beta, a_case, c_case, P, a_bufs, c_bufs, sa=None, a_axis=ROWS,
                           c_axis=None, rounding=FLOOR):
    """-> (expected C buffer of every rank in tc, SC[block, line] or None, t before the clamp or None);
    mx_common.expected_transform_mx with the FP6 codec"""
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
    q, E, t = quantise_dense6(V, c_axis, tc, rounding)
    out = mc.place(c_case, P, w6(q, tc), wc)
    return [narrow(o, tc) for o in out], E, t


def expected_tiles_mx6(ta, tc, sops, alpha, beta, a, c, m, n, sa=None, a_axis=ROWS, a_transposed=False,
                       c_axis=None, rounding=FLOOR, sc_fill=None):
    """mx_common.expected_tiles_mx with the FP6 codec; the ops' src / dst count ELEMENTS.
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
    q, E, tt = quantise_dense6(V, c_axis, tc, rounding)
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
    """every bit of the whole buffer (FP6 has no NaN; an expected fp32 NaN only asks for a NaN)"""
    if code == F:
        return mc.assert_bits(got, exp, F, what)
    g, e = np.ascontiguousarray(got, np.uint8).reshape(-1), np.ascontiguousarray(exp, np.uint8).reshape(-1)
    assert g.size == e.size, f"{what}: {g.size} bytes, {e.size} expected"
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} bytes differ, first at byte {bad[0]}: "
                           f"got {int(g[bad[0]]):#04x}, expected {int(e[bad[0]]):#04x}")


def assert_data_finite(exp, code, what):
    """no NaN and no inf expected, so assert_bits' "a NaN only asks for a NaN" rule hides nothing"""
    assert np.isfinite(widen(exp, code)).all(), f"{what}: the expected buffer holds a NaN or an inf"


# ------------------------------------------------------------------ the quad rule on exported ops
def op_quad(t, ta, tc):
    """the per-op half of the rule on one exported scaled op"""
    o = t["op"]
    nf, ns, lds, ldd, tr = int(o["nf"]), int(o["ns"]), int(o["lds"]), int(o["ldd"]), bool(int(o["flags"]) & 1)
    ok = True
    if ta in FP6:
        ok = ok and nf % 4 == 0 and lds % 4 == 0
    if tc in FP6:
        ok = ok and (ns if tr else nf) % 4 == 0 and ldd % 4 == 0
    return ok
