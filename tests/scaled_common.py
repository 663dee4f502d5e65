"""Shared by the scaled-transform tests (test_scaled_plan_cpu.py, test_gpu_scaled.py,
scaled_loopback_child.py): the 14 accepted pairs, conversions of every element type, scale vectors,
and the expected values.

Expected values come from the untouched CPU oracle only, in the compute type ct (float32; float64
for the DOUBLE pair).  For C(i, j) = beta*C(i, j) + alpha * ((op(A)(i, j) * r[i]) * c[j]):
  1. wa = A's buffer widened as the ordinary pair reads it (FLOAT -> H: w(cvt_H(a)));
  2. T = oracle.transform(ct, op, 1, 0, A -> zero buffers of C's layout): an exact redistribution;
  3. R, K = outer(r, 1), outer(1, c) distributed into C's layout (tri_common.distribute; fp32 values
     are exact in its float64), cast to ct;
  4. X = (T * R) * K in numpy ct: two rounded products, an absent vector skipped;
  5. oracle.transform(ct, "N", alpha, beta, C's layout: X -> w(c)), then cvt.
Tile lists the same way per op: the op's own source region is pre-scaled by its (row0, col0,
F_ROWS), then oracle.exec_tile_ops runs the plain ops.
"""
import numpy as np

import fp8_common as fc
import half_common as hc
import oracle
from half_common import geometry  # noqa: F401  (re-exported)
from tri_common import distribute

F, D, H16, BF16, E4M3, E5M2 = 0, 1, 5, 6, 7, 8
NAMES = {F: "f32", D: "f64", H16: "f16", BF16: "bf16", E4M3: "e4m3", E5M2: "e5m2"}
CNAMES = fc.CNAMES
ESIZE = fc.ESIZE
NPT = {F: np.float32, D: np.float64, H16: np.uint16, BF16: np.uint16, E4M3: np.uint8, E5M2: np.uint8}
# the 14 accepted pairs
PAIRS = [(F, F), (D, D)] + list(hc.PAIRS) + list(fc.PAIRS)
PAIR_IDS = [f"{NAMES[a]}-{NAMES[c]}" for a, c in PAIRS]
F_ROWS = 0x80
make_layout = fc.make_layout  # (its ESIZE knows every code)


def ctype(ta, tc):
    """numpy compute type of a pair"""
    return np.float64 if tc == D else np.float32


def ocode(ta, tc):
    return oracle.DOUBLE if tc == D else oracle.FLOAT


def _mod(code):
    return hc if code in (H16, BF16) else fc


def widen(b, code):
    if code == D:
        return np.ascontiguousarray(b, np.float64).copy()
    return _mod(code).widen(b, code)


def cvt(x, code):
    if code == D:
        return np.ascontiguousarray(x, np.float64).copy()
    return _mod(code).cvt(x, code)


def gen(code, seed, n):
    """n elements of `code` from the oracle's stream (|x| <= 1)"""
    if code == D:
        return oracle.gen(oracle.DOUBLE, seed, 0, n)
    return _mod(code).gen(code, seed, n)


def scales(n, seed, ct):
    """n scale values with |v| in [0.5, 2), mixed sign, random (non-power-of-two) mantissas"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 1.99, n) * rng.choice([-1.0, 1.0], n)
    v = v.astype(ct)
    assert ((np.abs(v) >= 0.5) & (np.abs(v) < 2)).all()
    return v


def source_values(a, ta, tc):
    """A's buffer as the pair delivers it to its arithmetic, in the compute type"""
    ct = ctype(ta, tc)
    if ta == F and tc in (H16, BF16):
        return hc.widen(hc.cvt(a, tc), tc).astype(ct)
    return widen(a, ta).astype(ct)


def assert_bits(got, exp, code, what):
    """raw bits over the whole buffer, except that an expected NaN only asks for a NaN"""
    if code != D:
        return _mod(code).assert_bits(got, exp, code, what)
    g = np.ascontiguousarray(got).view(np.uint64).reshape(-1)
    e = np.ascontiguousarray(exp).view(np.uint64).reshape(-1)
    assert g.size == e.size, f"{what}: {g.size} elements, {e.size} expected"
    nan = np.isnan(e.view(np.float64))
    assert np.isnan(g.view(np.float64)[nan]).all(), f"{what}: NaN expected"
    bad = np.flatnonzero((g != e) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} elements differ, first at {bad[0]}: "
                           f"got {int(g[bad[0]]):#x}, expected {int(e[bad[0]]):#x}")


def assert_finite(exp, code, what):
    """the expected buffer holds no NaN and no inf, so assert_bits' NaN rule hides nothing"""
    assert np.isfinite(widen(exp, code)).all(), f"{what}: the expected buffer holds a NaN or an inf"


def expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c, r=None, cs=None):
    """the whole expected C buffer (elements of tc) of a one-rank scaled transform"""
    ct, oc = ctype(ta, tc), ocode(ta, tc)
    wa = source_values(a, ta, tc)
    T = np.zeros(c_case.buf_elems(0, 1), ct)
    oracle.transform(oc, op, 1, 0, a_case.geom(1), [wa], c_case.geom(1), [T])
    m, n = c_case.shape()
    X = T
    if r is not None:
        assert r.size == m and r.dtype == ct
        X = X * distribute(np.outer(r.astype(np.float64), np.ones(n)), c_case, 1)[0].astype(ct)
    if cs is not None:
        assert cs.size == n and cs.dtype == ct
        X = X * distribute(np.outer(np.ones(m), cs.astype(np.float64)), c_case, 1)[0].astype(ct)
    assert X.dtype == ct
    wc = widen(c, tc).astype(ct)
    oracle.transform(oc, "N", alpha, beta, c_case.geom(1), [np.ascontiguousarray(X)], c_case.geom(1), [wc])
    return cvt(wc, tc)


def plain_ops(costa, sops):
    """the costa_tile_op_t part of scaled ops, without COSTA_SCALED_F_ROWS"""
    ops = np.ascontiguousarray(sops["op"]).copy()
    ops["flags"] &= ~np.uint32(F_ROWS)
    return ops


def op_coords(t):
    """target (i, j) of every source element (f, s) of one scaled op, both nf x ns"""
    nf, ns, flags = int(t["op"]["nf"]), int(t["op"]["ns"]), int(t["op"]["flags"])
    f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
    if flags & F_ROWS:
        return int(t["row0"]) + f, int(t["col0"]) + s
    return int(t["row0"]) + s, int(t["col0"]) + f


def expected_tiles(costa, ta, tc, sops, scal, a, c, r=None, cs=None):
    """the whole expected destination buffer of a scaled tile-op list whose `src` / `dst` offsets are
    in ELEMENTS; every op has its own source region"""
    ct, oc = ctype(ta, tc), ocode(ta, tc)
    wa = source_values(a, ta, tc)
    X = wa.copy()
    for t in sops:
        nf, ns, lds = int(t["op"]["nf"]), int(t["op"]["ns"]), int(t["op"]["lds"])
        f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
        idx = int(t["op"]["src"]) + s * lds + f
        i, j = op_coords(t)
        v = wa[idx]
        if r is not None:
            v = v * r[i]
        if cs is not None:
            v = v * cs[j]
        assert v.dtype == ct
        X[idx] = v
    wc = widen(c, tc).astype(ct)
    o = plain_ops(costa, sops)
    E = np.dtype(ct).itemsize
    o["src"] = o["src"] * E
    o["dst"] = o["dst"] * E
    oracle.exec_tile_ops(oc, o, np.asarray(scal, ct), X.ctypes.data, wc.ctypes.data)
    return cvt(wc, tc)
