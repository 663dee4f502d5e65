"""Shared by the amax tests (test_gpu_amax.py, amax_loopback_child.py): the expected row / column
amax vectors of tile lists, transforms and layouts, and their comparison.

costa_hip.h, "amax outputs": v[k] <- umax(bits(v[k]), absbits(x)) compared as the unsigned integer U
of the compute type's width, x the source value as the pair delivers it to its arithmetic.  The
expected vectors are built from the existing helpers only:
  tile lists   per op, i, j = scaled_common.op_coords(t) and v = absbits(source_values(...)[idx]);
               np.maximum.at on the U view of the initial vector
  transforms   T = oracle.transform(ct, op, 1, 0, wa -> zeros of C's layout), an exact
               redistribution of the source values; the row-index, column-index and ones matrices
               distributed into C's layout (tri_common.distribute) give (i, j, mask) per buffer
               element; then the same reduction
  layouts      the same with A's own layout and buffer, no transform
Vectors are compared as U over their whole length; an expected NaN only asks for a NaN (the
project's rule: device widening may quiet a payload), so every generic test also asserts that its
expected vectors hold no NaN, differ from the initial ones and are not constant (assert_moved).
"""
import numpy as np

import oracle
from scaled_common import D, cvt, ctype, gen, ocode, op_coords, source_values, widen
from tri_common import distribute


def utype(ct):
    return np.uint64 if np.dtype(ct) == np.float64 else np.uint32


def absbits(v):
    """the bits of a compute-type array with the sign bit cleared, as U"""
    v = np.ascontiguousarray(v)
    U = utype(v.dtype)
    return v.view(U) & U(np.iinfo(U).max >> 1)


def _update(vec, idx, vals):
    """vec (compute type, updated in place through its U view) <- umax(vec, absbits(vals)) at idx"""
    np.maximum.at(vec.view(utype(vec.dtype)), np.asarray(idx).reshape(-1), absbits(vals).reshape(-1))


def row_pow(i):
    """an exact power of two per global row (2^-2 .. 2^2) ..."""
    return np.ldexp(1.0, (np.asarray(i) * 7) % 5 - 2)


def col_pow(j):
    """... and per global column (2^-1 .. 2^2): a wrong index changes the answer"""
    return np.ldexp(1.0, (np.asarray(j) * 3) % 4 - 1)


_INDEX = {}


def layout_index(case, P=1):
    """per rank of `case` on P ranks: (global row, global column, inside the matrix, row_pow * col_pow)
    of every buffer element, computed once per layout (keyed by its spec) and left unchanged"""
    key = (case.spec(P), P)
    if key not in _INDEX:
        m, n = case.shape()
        ii = distribute(np.outer(np.arange(m), np.ones(n)), case, P)
        jj = distribute(np.outer(np.ones(m), np.arange(n)), case, P)
        mask = distribute(np.ones((m, n)), case, P)
        pw = distribute(np.outer(row_pow(np.arange(m)), col_pow(np.arange(n))), case, P)
        out = []
        for r in range(P):
            inside = mask[r] == 1
            out.append((ii[r].astype(np.int64), jj[r].astype(np.int64), inside, np.where(inside, pw[r], 1.0)))
            for a in out[-1]:
                a.setflags(write=False)
        _INDEX[key] = out
    return _INDEX[key]


def matrix_data(code, seed, case, P=1, rank=0):
    """rank's buffer of `case` in `code`: gen() values times row_pow(i) * col_pow(j) of the element's
    global position in the case's matrix; the padding keeps its gen() value"""
    pw = layout_index(case, P)[rank][3]
    g = gen(code, seed, case.buf_elems(rank, P))
    ct = np.float64 if code == D else np.float32
    return cvt((widen(g, code).astype(ct) * pw.astype(ct)).astype(ct), code)


def tile_data(code, seed, sops, n_src):
    """the source buffer of a tile list (offsets in elements): gen() values, each op's region times
    row_pow(i) * col_pow(j) of its target coordinates"""
    ct = np.float64 if code == D else np.float32
    w = widen(gen(code, seed, n_src), code).astype(ct)
    for t in sops:
        nf, ns, lds = int(t["op"]["nf"]), int(t["op"]["ns"]), int(t["op"]["lds"])
        f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
        idx = int(t["op"]["src"]) + s * lds + f
        i, j = op_coords(t)
        w[idx] = (w[idx] * (row_pow(i) * col_pow(j)).astype(ct)).astype(ct)
    return cvt(w, code)


def expected_tiles_amax(ta, tc, sops, a, row0, col0):
    """(row vector, column vector) after a tile list whose `src` offsets are in ELEMENTS ran on
    source buffer `a`, from the initial vectors row0 / col0 (compute type; None: not given)"""
    wa = source_values(a, ta, tc)
    r = None if row0 is None else row0.copy()
    c = None if col0 is None else col0.copy()
    for t in sops:
        nf, ns, lds = int(t["op"]["nf"]), int(t["op"]["ns"]), int(t["op"]["lds"])
        f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
        v = wa[int(t["op"]["src"]) + s * lds + f]
        i, j = op_coords(t)
        if r is not None:
            _update(r, i, v)
        if c is not None:
            _update(c, j, v)
    return r, c


def _reduce_layout(vals, case, P, rank, row0, col0):
    ii, jj, mask, _ = layout_index(case, P)[rank]
    assert vals.size == mask.size
    r = None if row0 is None else row0.copy()
    c = None if col0 is None else col0.copy()
    if r is not None:
        _update(r, ii[mask], vals[mask])
    if c is not None:
        _update(c, jj[mask], vals[mask])
    return r, c


def expected_transform_amax(ta, tc, op, a_case, c_case, a, row0, col0):
    """the vectors after a one-rank transform_amax of source buffer `a` (elements of ta)"""
    ct, oc = ctype(ta, tc), ocode(ta, tc)
    wa = source_values(a, ta, tc)
    T = np.zeros(c_case.buf_elems(0, 1), ct)
    oracle.transform(oc, op, 1, 0, a_case.geom(1), [wa], c_case.geom(1), [T])
    return _reduce_layout(T, c_case, 1, 0, row0, col0)


def expected_layout_amax(code, case, a, P, rank, row0, col0):
    """the vectors after layout_amax over rank's buffer `a` (elements of `code`) of `case`"""
    ct = np.float64 if code == D else np.float32
    return _reduce_layout(widen(a, code).astype(ct), case, P, rank, row0, col0)


def assert_vec(got, exp, what):
    """U over the whole vector, except that an expected NaN only asks for a NaN"""
    exp = np.ascontiguousarray(exp)
    got = np.ascontiguousarray(got).view(exp.dtype).reshape(-1)
    assert got.size == exp.size, f"{what}: {got.size} entries, {exp.size} expected"
    U = utype(exp.dtype)
    nan = np.isnan(exp)
    assert np.isnan(got[nan]).all(), f"{what}: NaN expected"
    g, e = got.view(U), exp.view(U)
    bad = np.flatnonzero((g != e) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} entries differ, first at {bad[0]}: "
                           f"got {int(g[bad[0]]):#x}, expected {int(e[bad[0]]):#x}")


def assert_moved(exp, init, what):
    """the expected vector holds no NaN, differs from the initial one and is not constant"""
    assert not np.isnan(exp).any(), f"{what}: the expected vector holds a NaN"
    assert exp.tobytes() != init.tobytes(), f"{what}: the expected vector equals the initial one"
    assert np.unique(exp.view(utype(exp.dtype))).size > 1, f"{what}: the expected vector is constant"
