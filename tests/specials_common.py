"""Shared by the special-value tests of the kernels' Annex G redo paths (test_gpu_tiles.py,
test_gpu_mixed.py, test_gpu_tri.py, test_gpu_parity.py, test_tile_variants_cpu.py).

The complex large shapes of tile_kernels.hip, convert_kernels.hip and tri_kernels.hip evaluate the
naive product, leave out the store of a strip (copy ops: V elements along f; transposing ops: V
along s, both counted from the sub-tile's origin) that holds an element whose result is NaN in both
parts, and recompute such strips element by element after the main loop.  The helpers
here say, on the host and from the data, the scalars and the oracle's expected buffer alone, which
strips that is and what the redo has to produce, so each test can assert that its data reaches the
code it is there for before any kernel runs.

`flagged` restates C99 Annex G's entry condition from the standard, as oracle/costa_oracle.c
ANNEX_G_MUL does; nothing here is read from the kernels' arithmetic.
"""
import ctypes
from collections import Counter, namedtuple

import numpy as np

import oracle

TR, CONJ, LE = 0x1, 0x2, 0x40
BITCOPY, ZERO, ALPHA, AXPBY = 0, 1, 2, 3
KIND = {ALPHA: "ALPHA", AXPBY: "AXPBY"}
# a test may accept "NaN on both sides" for at most this share of the real parts its ops write
NAN_CAP = 0.15

# the specials_c_big pair of the golden cases (tests/golden/cases.py) per real part type, and its
# real-typed counterpart
HUGE = {np.dtype(np.complex64): (1e30 + 1e30j, 2e25 - 1e25j), np.dtype(np.complex128): (1e300 + 1e300j, 2e295 - 1e295j),
        np.dtype(np.float32): (1e30, 2e25), np.dtype(np.float64): (1e300, 2e295)}


def real_type(dt):
    return np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64


def parts(a):
    """the buffer as its real parts, flat"""
    return np.ascontiguousarray(a).reshape(-1).view(real_type(a.dtype))


def assert_parts(got, exp, what):
    """every real part bit-equal, or NaN on both sides (NaNs the arithmetic generates differ in sign
    between x86 and the GPU, converted NaNs in payload): per part, over the whole buffer, so the
    finite or infinite part of a half-NaN element is compared too"""
    assert got.dtype == exp.dtype and got.size == exp.size, f"{what}: {got.dtype}[{got.size}] vs {exp.dtype}[{exp.size}]"
    g, e = parts(got), parts(exp)
    ut = np.uint32 if g.dtype == np.float32 else np.uint64
    bad = np.flatnonzero(np.where(np.isnan(e), ~np.isnan(g), g.view(ut) != e.view(ut)))
    if bad.size:
        per = g.size // got.size
        k = int(bad[0]) // per
        raise AssertionError(f"{what}: {bad.size} of {e.size} real parts differ, first in element {k}: "
                             f"got {got.reshape(-1)[k]!r}, expected {exp.reshape(-1)[k]!r}")


def written(ops, n_dst, E, kept=None):
    """mask over the destination's elements: those an op of the list writes (`kept(op)` -> nf x ns
    mask in (f, s) for masked ops)"""
    w = np.zeros(n_dst, bool)
    for op in ops:
        nf, ns, ldd = int(op["nf"]), int(op["ns"]), int(op["ldd"])
        f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
        idx = int(op["dst"]) // E + (f * ldd + s if int(op["flags"]) & TR else s * ldd + f)
        w[idx[kept(op)] if kept is not None else idx.reshape(-1)] = True
    return w


def assert_nan_share(exp, mask, what):
    """the share of NaN parts among the real parts the ops write stays under NAN_CAP, on the
    expected buffer (the reference alone is at a few percent) -> the share"""
    e = parts(exp).reshape(exp.size, -1)[mask]
    share = float(np.isnan(e).mean()) if e.size else 0.0
    assert share <= NAN_CAP, f"{what}: {share:.1%} of the written real parts are NaN, the cap is {NAN_CAP:.0%}"
    return share


def _at(addr, n, dt):
    """n elements of host memory at an address, as an array"""
    return np.frombuffer((ctypes.c_char * (n * np.dtype(dt).itemsize)).from_address(addr), dt)


def exec_ops(code, ops, scal, src_base=0, dst_base=0):
    """oracle.exec_tile_ops with every op evaluated as the scale kind it carries (costa_hip.h:
    g(x) = x for BITCOPY, alpha * op(x) for ALPHA).  The oracle chooses its branch from the scalars
    as the reference does, and the planner derives the kind by the same rule (plan.cpp scale_kind,
    tile_op.hpp tile_op), so the two agree on every op a plan holds.  The hand-made lists also hold
    two forms no plan holds, which the kernels run as listed and the oracle's rule would swap:
      * ALPHA with alpha = 1, beta = 0 on a copy op without conjugation: the product 1 * x (the
        oracle's rule: memcpy).  Run here as a transposing op of the oracle, whose alpha = 1 is a
        product, into a scratch tile that is then copied to its place.
      * BITCOPY on a transposing op: the bytes, transposed (the oracle's rule: the product 1 * x).
    On finite data both forms give the same bytes either way (the existing list tests); on complex
    inf / NaN / -0 they do not: (1 + 0i)(inf + 2i) = inf + NaN i."""
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    sc = np.ascontiguousarray(scal, dt).reshape(-1)
    for op in ops:
        flags = int(op["flags"])
        kind, slot, tr, conj = flags >> 4 & 3, flags >> 16, flags & TR, flags & CONJ
        nf, ns, lds, ldd = (int(op[k]) for k in ("nf", "ns", "lds", "ldd"))
        unit = kind == ALPHA and sc[2 * slot] == 1 and sc[2 * slot + 1] == 0
        if not ((unit and not tr and not conj) or (kind == BITCOPY and tr)) or nf * ns == 0:
            oracle.exec_tile_ops(code, op.reshape(1), sc, src_base, dst_base)
            continue
        assert not conj
        x = _at(src_base + int(op["src"]), (ns - 1) * lds + nf, dt)
        f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
        if kind == BITCOPY:
            d = _at(dst_base + int(op["dst"]), (nf - 1) * ldd + ns, dt)
            d.view(f"V{E}")[f * ldd + s] = x.view(f"V{E}")[s * lds + f]
        else:
            tile = np.empty(nf * ns, dt)
            oracle.copy_and_transform(code, nf, ns, x, lds, True, tile, ns, True, transpose=True, alpha=1, beta=0)
            d = _at(dst_base + int(op["dst"]), (ns - 1) * ldd + nf, dt)
            d.view(f"V{E}")[s * ldd + f] = tile.view(f"V{E}").reshape(nf, ns)


def _cparts(z, rt):
    z = np.asarray(z)
    return z.real.astype(rt), z.imag.astype(rt)


def flagged(kind, conj, alpha, beta, x, y=None):
    """C99 Annex G's entry condition per element: both parts of the naive result NaN, computed in
    the element's own real type.  x' = conj(x) if conj, p = (ar*x'r - ai*x'i, ar*x'i + ai*x'r); AXPBY
    adds q = beta*y computed the same way: (qr + pr, qi + pi).  Other kinds multiply nothing."""
    x = np.asarray(x)
    if kind not in (ALPHA, AXPBY):
        return np.zeros(x.shape, bool)
    rt = real_type(x.dtype)
    with np.errstate(all="ignore"):
        xr, xi = _cparts(x, rt)
        if conj:
            xi = -xi
        ar, ai = (rt(v) for v in (np.real(alpha), np.imag(alpha)))
        pr, pi = ar * xr - ai * xi, ar * xi + ai * xr
        if kind == AXPBY:
            yr, yi = _cparts(y, rt)
            br, bi = (rt(v) for v in (np.real(beta), np.imag(beta)))
            qr, qi = br * yr - bi * yi, br * yi + bi * yr
            pr, pi = qr + pr, qi + pi
    return np.isnan(pr) & np.isnan(pi)


def _both_nan(z):
    return np.isnan(z.real) & np.isnan(z.imag)


def _any_inf(z):
    return np.isinf(z.real) | np.isinf(z.imag)


# one sub-tile of a shaped launch: the op (src / dst in bytes from the buffers' starts), the
# sub-tile's origin and extent in (f, s), the kernel's whole / guarded verdict and the launch's name
Sub = namedtuple("Sub", "launch op f0 s0 tf ts whole")
COUNTS = ("redone", "recovered", "not_redone", "mixed", "partial", "overflow", "straddle")


def redo_cells(subs, src, dst0, exp, scal, V, kept=None):
    """-> {(launch, "whole" | "guarded", "tr" | "copy", "ALPHA" | "AXPBY", "conj" | "plain"): Counter}
    over the complex ALPHA / AXPBY sub-tiles of `subs`, counted from the data (src already in the
    destination's type), the slot scalars and the oracle's expected buffer:
      redone      strips holding at least one flagged element
      recovered   flagged elements whose expected value is not NaN in both parts
      not_redone  strips (with an element the op writes) holding no flagged element
      mixed       redone strips that also hold an unflagged element with a finite expected value
      partial     redone strips with fewer than V elements inside the sub-tile
      overflow    recovered elements with no infinite input part (the overflow branch)
      straddle    masked ops: redone strips that also hold a dropped element
    A strip is V consecutive elements from the sub-tile's origin, along f for copy ops and along s
    for transposing ops.  kept(op) -> nf x ns mask in (f, s) of a masked op's written elements"""
    E = dst0.itemsize
    cells = {}
    masks = {}
    for sub in subs:
        op = sub.op
        flags = int(op["flags"])
        kind = flags >> 4 & 3
        if kind not in KIND:
            continue
        tr, conj, slot = bool(flags & TR), bool(flags & CONJ), flags >> 16
        alpha, beta = scal[2 * slot], scal[2 * slot + 1]
        f = sub.f0 + np.arange(sub.tf)[:, None]
        s = sub.s0 + np.arange(sub.ts)[None, :]
        x = src[int(op["src"]) // E + s * int(op["lds"]) + f]
        didx = int(op["dst"]) // E + (f * int(op["ldd"]) + s if tr else s * int(op["ldd"]) + f)
        y, e = dst0[didx], exp[didx]
        if kept is None:
            keep = np.ones(x.shape, bool)
        else:
            key = (int(op["src"]), int(op["dst"]))  # (every op has its own region of both buffers)
            if key not in masks:
                masks[key] = kept(op)
            keep = masks[key][sub.f0:sub.f0 + sub.tf, sub.s0:sub.s0 + sub.ts]
        fl = flagged(kind, conj, alpha, beta, x, y) & keep
        rec = fl & ~_both_nan(e)
        fin = keep & ~fl & np.isfinite(e.real) & np.isfinite(e.imag)
        noinf = ~_any_inf(x) & ~np.isinf(alpha.real) & ~np.isinf(alpha.imag)
        if kind == AXPBY:
            noinf &= ~_any_inf(y)
        axis, n = (1, sub.ts) if tr else (0, sub.tf)
        at = np.arange(0, n, V)
        strip = lambda m: np.logical_or.reduceat(m, at, axis=axis)  # noqa: E731
        hit, live = strip(fl), strip(keep)
        short = np.zeros(hit.shape, bool)
        if n % V:
            (short[:, -1:] if tr else short[-1:, :])[...] = True
        c = cells.setdefault((sub.launch, "whole" if sub.whole else "guarded", "tr" if tr else "copy",
                              KIND[kind], "conj" if conj else "plain"), Counter(dict.fromkeys(COUNTS, 0)))
        c["redone"] += int(hit.sum())
        c["recovered"] += int(rec.sum())
        c["not_redone"] += int((live & ~hit).sum())
        c["mixed"] += int((hit & strip(fin)).sum())
        c["partial"] += int((hit & short).sum())
        c["overflow"] += int((rec & noinf).sum())
        c["straddle"] += int((hit & strip(~keep)).sum())
    return cells


def total(cells, **want):
    """the sum of the cells whose key matches: launch=, fill= ("whole" / "guarded"), mode= ("tr" /
    "copy"), kind=, conj="""
    names = ("launch", "fill", "mode", "kind", "conj")
    assert set(want) <= set(names), want
    out = Counter(dict.fromkeys(COUNTS, 0))
    for key, c in cells.items():
        if all(key[names.index(k)] == v for k, v in want.items()):
            out.update(c)
    return out


def strip_subs(launch, ops, bf, bs, whole_of):
    """every sub-tile of every op of a strip-kernel list (strip_work.hpp build_strip_work lists the
    bf x bs sub-tiles of each op in turn); whole_of(op, f0, s0, tf, ts) -> the kernel's verdict, or
    None for a sub-tile the builder leaves out"""
    for op in ops:
        nf, ns = int(op["nf"]), int(op["ns"])
        for s0 in range(0, ns, bs):
            for f0 in range(0, nf, bf):
                tf, ts = min(bf, nf - f0), min(bs, ns - s0)
                w = whole_of(op, f0, s0, tf, ts)
                if w is not None:
                    yield Sub(launch, op, f0, s0, tf, ts, bool(w))
