"""MXFP6 on the GPU (costa_hip.h, "MXFP6"): the packed e2m3 / e3m2 instantiations of mx_kernel through
costa_hip_execute_tiles_mx, and costa_hip_transform_mx on one rank, on a stream, on emulated ranks and
through the loopback exchange.  Expected packed bytes and scale bytes come from the numpy model of
fp6_common.py; every comparison is exact and covers the whole destination buffer: neighbouring
groups, ld padding and the gaps between block buffers keep their fill."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fp6_common as f6
import mx_common as mc
import oracle
from emulated_ranks import drive
from fp6_common import CEIL, COLS, E2M3, E3M2, F, FLOOR, FP6, NAMES, ROWS, assert_same, make_layout
from test_gpu_mx import ScaleT, dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR, F_ROWS = 0x1, 0x80
BITCOPY, ALPHA, AXPBY = 0, 2, 3
NPT = {F: np.float32, E2M3: np.uint8, E3M2: np.uint8}
RND = {FLOOR: "floor", CEIL: "ceil"}
M, N = 204, 156          # 6 * 32 + 12 and 4 * 32 + 28
TYPES = pytest.mark.parametrize("p", FP6, ids=[NAMES[p] for p in FP6])
# alpha of the requantise tests: turns the largest magnitudes fmax * 2^k into 1.03125 * fmax * 2^k, above
# fmax after the floor rule's scaling, so the clamp runs (a power of two times an FP6 value alone never
# lands above fmax)
ALPHA_RQ = 1.03125


def kinds(p):
    return {"quantise": (F, p), "dequantise": (p, F), "requantise": (p, p)}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def host(t, code):
    return t.cpu().numpy().view(NPT[code])


# ------------------------------------------------------------------ kernel level: tile lists
def _regions(axis):
    """target regions (row0, col0, rows, cols, F_ROWS, source ld rule, destination ld rule, offset) of the
    204 x 156 matrix; every extent is a multiple of 4 (the quad rule holds on either side, copy or
    transpose).  Along the block axis (length L) every op starts on a multiple of 32 and ends on one or at
    the matrix edge, where the last MX block is partial: 12 of 32 rows, 28 of 32 columns.
    ld rules: 'v' a multiple of 32 (a byte pitch that is a multiple of 24), 'b' 204 (= 4 mod 8: a byte
    pitch of 153, so consecutive lines alternate parity); offset 4 puts the first element of an FP6 side
    3 bytes in, on an odd byte.  Every list holds whole 64 x 64 sub-tiles on aligned sides (FULL path), a
    remainder of 12 along f and one of 28 along s (guarded path)."""
    L, O = (M, N) if axis == ROWS else (N, M)
    reg = [
        (0, 0, 64, 64, True, "v", "v", 0),          # one whole sub-tile, blocks along f (FULL path)
        (64, 0, 64, 64, False, "v", "v", 0),        # one whole sub-tile, blocks along s (FULL path)
        (128, 0, L - 128, 44, True, "b", "v", 0),   # up to the edge along f (rows: 64 + 12), a partial block
        (128, 44, L - 128, 28, False, "v", "b", 0),  # the same with the blocks along s; 28 = 7 strips
        (0, 64, 96, O - 64, True, "b", "b", 0),     # 96 x 92 (140): remainder sub-tiles on both sides
        (96, 64, 32, 20, False, "v", "v", 4),       # aligned ld, first element on an odd byte
        (128, 72, L - 128, 12, False, "b", "b", 4),  # 12 along f, 76 (28) along s; ld = 4 mod 8 on an odd byte
    ]
    out = []
    for b0, o0, nb, no, along_f, sl, dl, off in reg:
        if axis == ROWS:
            out.append((b0, o0, nb, no, along_f, sl, dl, off))
        else:
            out.append((o0, b0, no, nb, not along_f, sl, dl, off))
    return out


def _tile_list(costa, axis, transpose, kind, slot=0):
    """-> (ops with ELEMENT offsets, source elements, destination elements)"""
    regions = _regions(axis)
    ops = np.zeros(len(regions), costa.SCALED_OP_DTYPE)
    src_at = dst_at = 0
    rem_f = rem_s = False
    for k, (r0, c0, nr, nc, frow, sl, dl, off) in enumerate(regions):
        nf, ns = (nr, nc) if frow else (nc, nr)
        assert nf % 4 == 0 and ns % 4 == 0
        rem_f, rem_s = rem_f or nf % 64 == 12, rem_s or ns % 64 == 28

        def place(at, fast, slow, rule, off):
            ld = (fast + 31) // 32 * 32 if rule == "v" else 204
            assert ld >= fast and ld % 4 == 0
            return at + off, ld, (at + off + ld * slow + 31) // 32 * 32
        s0, lds, src_at = place(src_at, nf, ns, sl, off)
        df, dslow = (ns, nf) if transpose else (nf, ns)
        d0, ldd, dst_at = place(dst_at, df, dslow, dl, off)
        flags = (TR if transpose else 0) | kind << 4 | slot << 16 | (F_ROWS if frow else 0)
        ops[k] = ((s0, d0, nf, ns, lds, ldd, flags, 0), r0, c0)
    assert rem_f and rem_s, "the list holds no remainder of 12 along f or of 28 along s"
    return ops, src_at + 32, dst_at + 32


def _subtiles(ops):
    return sum(-(-int(o["op"]["nf"]) // 64) * -(-int(o["op"]["ns"]) // 64) for o in ops)


def _gpu_ops(ops, ta, tc):
    """element offsets -> byte offsets (4 per fp32 element, 3 per 4 FP6 elements)"""
    g = ops.copy()
    for side, code in (("src", ta), ("dst", tc)):
        assert code == F or (ops["op"][side] % 4 == 0).all()
        g["op"][side] = ops["op"][side] * 4 if code == F else ops["op"][side] * 3 // 4
    if ta != F or tc != F:
        fp6_at = np.concatenate([g["op"][s] for s, code in (("src", ta), ("dst", tc)) if code != F])
        assert len(ops) < 3 or (fp6_at % 2 == 1).any(), "no op starts on an odd byte of its FP6 side"
    return g


def _run_tiles(costa, ta, tc, ops, n_src, n_dst, m, n, alpha, beta, a_axis, c_axis, order, rounding, a_tr, what,
               src=None, sa=None, finite=True):
    scal = np.array([alpha, beta], np.float32)
    if src is None:
        src = mc.quant_data(0xA1, n_src) if ta == F else f6.fp6_data(0xA2, n_src)
    dst0 = f6.fill(tc, 0xC1, n_dst)
    SA = SC = None
    if ta != F:
        am, an = (n, m) if a_tr else (m, n)
        shape = (mc.n_blocks(am), an) if a_axis == ROWS else (mc.n_blocks(an), am)
        SA = ScaleT(costa, a_axis, *shape, order, init=mc.scale_bytes(0x5A, shape) if sa is None else sa)
    if tc != F:
        shape = (mc.n_blocks(m), n) if c_axis == ROWS else (mc.n_blocks(n), m)
        SC = ScaleT(costa, c_axis, *shape, order)
    exp, esc, t = f6.expected_tiles_mx6(ta, tc, ops, alpha, beta, src, dst0, m, n, sa=SA.init if SA else None,
                                        a_axis=a_axis, a_transposed=a_tr, c_axis=c_axis if SC else None,
                                        rounding=rounding, sc_fill=SC.init if SC else None)
    if finite:
        f6.assert_data_finite(exp, tc, what)
    ds, dd = dev(src), dev(dst0)
    assert ds.numel() == f6.buf_bytes(ta, n_src) and dd.numel() == f6.buf_bytes(tc, n_dst)
    i0, s0, a0 = costa.mx_items(), costa.scaled_items(), costa.amax_items()
    costa.execute_tiles_mx(ta, tc, _gpu_ops(ops, ta, tc), scal, m, n, ds.data_ptr(), dd.data_ptr(),
                           a_scales=SA.desc if SA else None, c_scales=SC.desc if SC else None,
                           rounding=RND[rounding], a_transposed=a_tr)
    got = host(dd, tc)
    if SC:
        SC.check(esc, what + ": c_scales")
    if SA:
        SA.check(SA.init, what + ": a_scales")
    assert_same(got, exp, tc, what + ": destination")
    assert costa.mx_items() - i0 == _subtiles(ops)
    assert costa.scaled_items() == s0 and costa.amax_items() == a0
    assert ds.cpu().numpy().tobytes() == np.ascontiguousarray(src).tobytes()
    return got, exp, esc, t


def _check_saturation(exp, t, p, rounding, what):
    codes = f6.unpack(exp)
    if rounding == FLOOR:  # the clamp ran: values above fmax before it, the saturating code stored
        assert (np.abs(t) > f6.FMAX[p]).any(), what
        assert ((codes & 31) == 31).any(), what
    else:
        assert (np.abs(t) <= f6.FMAX[p]).all(), what


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("order", ["block", "line"])
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@TYPES
def test_quantise_tile_lists(costa, p, transpose, axis, order, rounding):
    what = f"quantise f32->{NAMES[p]} {'tr' if transpose else 'copy'} axis {axis} {order} {RND[rounding]}"
    kind, alpha = (ALPHA, -0.5) if transpose or rounding == CEIL else (BITCOPY, 1.0)
    lst = _tile_list(costa, axis, transpose, kind)
    got, exp, esc, t = _run_tiles(costa, F, p, *lst, M, N, alpha, 0.0, None, axis, order, rounding, False, what)
    _check_saturation(exp, t, p, rounding, what)


@pytest.mark.parametrize("order", ["block", "line"])
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("a_tr", [False, True], ids=["a", "at"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_dequantise_tile_lists(costa, transpose, a_tr, axis, order):
    """beta != 0: the old destination values are read; a_scales indexed by A's matrix, also turned round"""
    p = E2M3 if (axis == ROWS) == (order == "block") else E3M2
    what = f"dequantise {NAMES[p]}->f32 {'tr' if transpose else 'copy'} a_tr {a_tr} axis {axis} {order}"
    lst = _tile_list(costa, ROWS if transpose else COLS, transpose, AXPBY)
    got, exp, _, _ = _run_tiles(costa, p, F, *lst, M, N, -0.5, 2.0, axis, None, order, FLOOR, a_tr, what)
    assert np.isfinite(exp).all()


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("axes", [(ROWS, COLS), (COLS, ROWS), (ROWS, ROWS), (COLS, COLS)],
                         ids=["rows-cols", "cols-rows", "rows-rows", "cols-cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_requantise_tile_lists(costa, transpose, axes, rounding):
    a_axis, c_axis = axes
    p = E2M3 if (a_axis == c_axis) == (rounding == FLOOR) else E3M2
    what = f"requantise {NAMES[p]} {'tr' if transpose else 'copy'} axes {axes} {RND[rounding]}"
    order = "block" if rounding == FLOOR else "line"
    lst = _tile_list(costa, c_axis, transpose, ALPHA)
    got, exp, esc, t = _run_tiles(costa, p, p, *lst, M, N, ALPHA_RQ, 0.0, a_axis, c_axis, order, rounding, transpose,
                                  what)
    _check_saturation(exp, t, p, rounding, what)


# ------------------------------------------------------------------ specials
N_SPECIAL = 12


def _special_blocks(p):
    """one block per column of a 32 x 12 matrix (blocks along rows)"""
    fm = f6.FMAX[p]
    top = fm * np.float32(8.0 if p == E2M3 else 2.0)                   # 60 / 56: in [32, 64), e = 127 + 5
    assert 40 < top < 64
    ties = np.array([mid for mid, _ in f6.TIES[p]], np.float32)
    V = np.zeros((32, N_SPECIAL), np.float32)
    V[[2, 11, 30], 0] = -0.0                                           # all zero, some -0
    V[:, 1] = -0.5
    V[9, 1] = np.inf                                                   # an inf
    V[:, 2] = 0.25
    V[9, 2] = np.nan                                                   # a NaN
    V[:, 3] = np.float32(2.0 ** -127) * np.linspace(-1, 1, 32, dtype=np.float32)   # maximum below 2^-125
    V[:, 4] = np.float32(2.5e38) * np.linspace(-1, 1, 32, dtype=np.float32)        # maximum near 2^127
    V[:, 5] = np.linspace(-40, 40, 32, dtype=np.float32)
    V[5, 5] = top                                                      # scales to exactly fmax
    V[:, 6] = V[:, 5]
    V[5, 6] = np.nextafter(top, np.float32(64.0))                      # just above: ceil raises E, floor saturates
    V[:31, 7] = ties * np.float32(2.0 ** -4)                           # the 31 ties at one scale
    V[:31, 8] = -ties * np.float32(2.0 ** -4)
    V[:, 9] = np.finfo(np.float32).max * np.linspace(-1, 1, 32, dtype=np.float32)  # the largest E there is
    return V                                                           # (columns 10, 11: all +0)


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("frow", [True, False], ids=["along-f", "along-s"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@TYPES
def test_special_blocks(costa, p, transpose, frow, rounding):
    V = _special_blocks(p)
    m, n = V.shape
    emax = f6.EMAX[p]
    src = (V.T if frow else V).reshape(-1).copy()  # element (f, s) at s * lds + f
    nf, ns = (m, n) if frow else (n, m)
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ldd = ns if transpose else nf
    ops[0] = ((0, 0, nf, ns, nf, ldd, (TR if transpose else 0) | BITCOPY << 4 | (F_ROWS if frow else 0), 0), 0, 0)
    what = f"specials {NAMES[p]} {'tr' if transpose else 'copy'} frow {frow} {RND[rounding]}"
    got, exp, esc, t = _run_tiles(costa, F, p, ops, src.size, m * n, m, n, 1.0, 0.0, None, ROWS, "block", rounding,
                                  False, what, src=src, finite=False)
    # by hand: the inf block and the NaN block, 32 elements each, are all NaN before the clamp; nothing else
    assert int(np.isnan(t).sum()) == 2 * 32 and np.isnan(t[:, 1]).all() and np.isnan(t[:, 2]).all()
    up = 1 if rounding == CEIL else 0
    E = esc[0]
    assert E[0] == 0 and E[1] == 255 and E[2] == 255 and E[3] == 0 and E[4] == 254 - emax
    assert E[5] == 127 + 5 - emax and E[6] == 127 + 5 - emax + up and E[7] == 123 and E[8] == 123
    assert E[9] == 254 - emax + up and E[10] == 0 and E[11] == 0       # FLT_MAX scales to 1.99.. * 2^emax > fmax
    # the codes of the target matrix, whatever the destination's orientation
    codes = f6.unpack(got).reshape((m, n) if transpose == frow else (n, m))
    Q = codes if transpose == frow else codes.T
    assert (Q[:, 1] == 0).all() and (Q[:, 2] == 0).all()               # E = 255: code 0x00 everywhere
    assert list(Q[[2, 11, 30], 0]) == [0x20] * 3 and (np.delete(Q[:, 0], [2, 11, 30]) == 0).all()
    half = f6.cvt6(np.array([f6.FMAX[p] / 2], np.float32), p)[0]
    assert Q[5, 5] == 0x1F and Q[5, 6] == (0x1F if rounding == FLOOR else half)
    k = np.arange(31)
    even = np.where(k % 2 == 0, k, k + 1)
    assert list(Q[:31, 7]) == list(even) and list(Q[:31, 8]) == list(even | 0x20)
    # column 3 lands in the subnormal range of the type (and below it: zeros that keep their sign)
    sub = Q[:, 3] & 31
    assert ((sub > 0) & (sub < (8 if p == E2M3 else 4))).any() and Q[0, 3] & 0x20
    assert (Q[:, 10] == 0).all() and (Q[:, 11] == 0).all()


# ------------------------------------------------------------------ exhaustive dequantise
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@TYPES
def test_every_code_against_the_special_scale_bytes(costa, p, transpose, axis):
    """all 64 codes times the scale bytes 0, 1, 126, 127, 128, 254, 255: subnormal products are kept, 255
    makes NaNs, -0 keeps its sign.  The source is 56 lines of 64 elements with the blocks along the lines
    (f): line s holds all 64 codes, rotated by s, and meets the scale byte number s % 7 in both of its
    blocks, so the 56 lines give every (code, scale byte) pair."""
    nf, ns = 64, 56
    vals = np.array([0, 1, 126, 127, 128, 254, 255], np.uint8)
    frow = axis == ROWS                        # the blocks run along f: f walks rows for ROWS, columns for COLS
    m, n = (nf, ns) if frow else (ns, nf)
    sa = np.broadcast_to(vals[np.arange(ns) % 7][None, :], (2, ns)).copy()      # [block, line]
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, nf, ns, nf, ns if transpose else nf, (TR if transpose else 0) | ALPHA << 4 | (F_ROWS if frow else 0),
               0), 0, 0)
    f, s_ = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
    codes = np.zeros(nf * ns, np.uint8)
    codes[s_ * nf + f] = (f + s_) % 64
    met = codes[s_ * nf + f].astype(np.int64) * 256 + sa[f // 32, s_]
    assert np.unique(met).size == 64 * vals.size
    what = f"every code {NAMES[p]} {'tr' if transpose else 'copy'} axis {axis}"
    got, exp, _, _ = _run_tiles(costa, p, F, ops, nf * ns, nf * ns, m, n, 1.0, 0.0, axis, None, "line", FLOOR, False,
                                what, src=f6.pack(codes), sa=sa, finite=False)
    # by hand: a scale byte of 255 makes every element of its line a NaN (0 * NaN too): 56 / 7 lines of 64;
    # 254 (2^127) takes the magnitudes from 2.0 up (codes 16 .. 31 of either type, both signs) to inf
    assert int(np.isnan(exp).sum()) == (ns // 7) * nf and int(np.isinf(exp).sum()) == (ns // 7) * 32
    sub = exp[(exp != 0) & np.isfinite(exp) & (np.abs(exp) < 2.0 ** -126)]
    assert sub.size > 0 and (np.signbit(exp) & (exp == 0)).any()


# ------------------------------------------------------------------ transform_mx on one rank
def _scales_for(costa, case_shape, axis, order, init=None, fill=0xA5):
    rows, cols = case_shape
    shape = (mc.n_blocks(rows), cols) if axis == ROWS else (mc.n_blocks(cols), rows)
    return ScaleT(costa, axis, *shape, order, init=None if init is None else init(shape), fill=fill)


def _xf(costa, p, kind, geom, op, a_axis=ROWS, c_axis=ROWS, rounding=FLOOR, alpha=1.0, beta=0.0, order="block",
        stream=None, comm=None):
    """one one-rank transform_mx against the model -> t before the clamp"""
    ta, tc = kinds(p)[kind]
    a_case, c_case = f6.geometry(geom, op)
    what = f"{kind} {NAMES[ta]}->{NAMES[tc]} {geom} {op}"
    na, nc = a_case.buf_elems(0, 1), c_case.buf_elems(0, 1)
    a = mc.quant_data(0x31, na) if ta == F else f6.fp6_data(0x32, na)
    c = f6.fill(tc, 0x33, nc)
    SA = _scales_for(costa, a_case.shape(), a_axis, order, lambda s: mc.scale_bytes(0x34, s)) if ta != F else None
    SC = _scales_for(costa, c_case.shape(), c_axis, order) if tc != F else None
    exp, esc, t = f6.expected_transform_mx6(ta, tc, op, alpha, beta, a_case, c_case, 1, [a], [c],
                                            sa=SA.init if SA else None, a_axis=a_axis,
                                            c_axis=c_axis if SC else None, rounding=rounding)
    f6.assert_data_finite(exp[0], tc, what)
    da, dc = dev(a), dev(c)
    assert da.numel() == f6.buf_bytes(ta, na) and dc.numel() == f6.buf_bytes(tc, nc)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    comm = comm or costa.Comm.self(0)
    i0, s0 = costa.mx_items(), costa.scaled_items()
    costa.transform_mx(A, C, comm, op, alpha, beta, a_scales=SA.desc if SA else None,
                       c_scales=SC.desc if SC else None, rounding=RND[rounding], stream=stream)
    if stream is not None:
        stream.synchronize()
    if SC:
        SC.check(esc, what + ": c_scales")
    if SA:
        SA.check(SA.init, what + ": a_scales")
    assert_same(host(dc, tc), exp[0], tc, what)
    assert da.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    assert costa.mx_items() > i0 and costa.scaled_items() == s0
    return t


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", f6.GEOMETRIES)
@pytest.mark.parametrize("kind", ["quantise", "dequantise", "requantise"])
def test_transform_mx_one_rank(costa, kind, geom, op):
    # the type and the axes alternate with the geometry
    p = E3M2 if geom == "g204pad" else E2M3
    rounding = CEIL if geom == "g204pad" else FLOOR
    # requantise 'T' turns the block axis round ('N' keeps it); the others alternate with the geometry
    a_axis = ROWS if geom in ("g204", "custom32q") else COLS
    c_axis = (COLS if a_axis == ROWS else ROWS) if kind == "requantise" and op == "T" else a_axis
    alpha, beta = (-0.5, 2.0) if kind == "dequantise" and op == "T" else (1.0, 0.0) if op == "N" else (ALPHA_RQ, 0.0)
    t = _xf(costa, p, kind, geom, op, a_axis, c_axis, rounding, alpha, beta, order="block" if op == "N" else "line")
    if kind == "quantise":
        if rounding == FLOOR:
            assert (np.abs(t) > f6.FMAX[p]).any()
        else:
            assert (np.abs(t) <= f6.FMAX[p]).all()


@pytest.mark.parametrize("axis,want", [(ROWS, {E2M3: 1208, E3M2: 2446}), (COLS, {E2M3: 227, E3M2: 472})],
                         ids=["rows", "cols"])
@TYPES
def test_quantise_saturation_counts(costa, p, axis, want):
    """quant_data at 204 x 156, seed 0x31: the number of elements above fmax before the clamp under the
    floor rule, and none under ceil"""
    t = _xf(costa, p, "quantise", "g204", "N", c_axis=axis)
    assert int((np.abs(t) > f6.FMAX[p]).sum()) == want[p]
    t = _xf(costa, p, "quantise", "g204", "N", c_axis=axis, rounding=CEIL)
    assert int((np.abs(t) > f6.FMAX[p]).sum()) == 0


def test_requantise_transposed_keeps_cols_blocks(costa):
    """'T' from axis COLS of A to axis COLS of the transposed matrix: no byte tool can do it (every code
    moves to another bit position), the model dequantises and requantises"""
    _xf(costa, E3M2, "requantise", "g204", "T", a_axis=COLS, c_axis=COLS, alpha=ALPHA_RQ)


def test_transform_mx_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _xf(costa, E2M3, "quantise", "g204", "T", c_axis=COLS, alpha=0.75, stream=s)
        _xf(costa, E2M3, "dequantise", "g204", "T", a_axis=COLS, alpha=0.75, stream=s)


# ------------------------------------------------------------------ several ranks on one GPU
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", ["quantise", "dequantise"])
def test_emulated_ranks_2x2(costa, kind, op):
    """quantise sends fp32 packages, dequantise packed FP6 packages counted in bytes; each rank's c_scales
    holds exactly its own blocks' bytes over a zero fill and their maximum is the model's tensor"""
    P = 4
    p = E2M3 if op == "N" else E3M2
    ta, tc = kinds(p)[kind]
    a_case, c_case = f6.geometry("g204", op, (2, 2))
    m, n = c_case.shape()
    alpha, beta = (0.75, 0.0) if kind == "quantise" else (-0.5, 2.0)
    a = [mc.quant_data(0x40 + r, a_case.buf_elems(r, P)) if ta == F else f6.fp6_data(0x40 + r, a_case.buf_elems(r, P))
         for r in range(P)]
    c = [f6.fill(tc, 0x50 + r, c_case.buf_elems(r, P)) for r in range(P)]
    axis = COLS if op == "T" else ROWS
    am, an = a_case.shape()
    sa_shape = (mc.n_blocks(am), an) if axis == ROWS else (mc.n_blocks(an), am)
    sc_shape = (mc.n_blocks(m), n) if axis == ROWS else (mc.n_blocks(n), m)
    sa = mc.scale_bytes(0x66, sa_shape) if ta != F else None
    exp, esc, _ = f6.expected_transform_mx6(ta, tc, op, alpha, beta, a_case, c_case, P, a, c, sa=sa, a_axis=axis,
                                            c_axis=axis if tc != F else None)
    for r in range(P):
        f6.assert_data_finite(exp[r], tc, f"{kind} {op} rank {r}")
    da, dc = [dev(x) for x in a], [dev(x) for x in c]
    lay = [(make_layout(costa, a_case, r, da[r].data_ptr(), P, ta), make_layout(costa, c_case, r, dc[r].data_ptr(), P, tc))
           for r in range(P)]
    plans = [costa.plan_export_scaled(lay[r][0], lay[r][1], r, P, op, alpha, beta) for r in range(P)]
    assert all(q.send_elems > 0 and q.recv_elems > 0 for q in plans)
    SA = [ScaleT(costa, axis, *sa_shape, "line", init=sa) if ta != F else None for r in range(P)]
    SC = [ScaleT(costa, axis, *sc_shape, "block", fill=0) if tc != F else None for r in range(P)]
    i0, s0 = costa.mx_items(), costa.scaled_items()

    def call(r, comm):
        costa.transform_mx(lay[r][0], lay[r][1], comm, op, alpha, beta, a_scales=SA[r].desc if SA[r] else None,
                           c_scales=SC[r].desc if SC[r] else None)

    # bytes of a package unit: an fp32 element, or one byte of a packed package
    out = drive(costa, plans, 4 if ta == F else 1, call)
    assert out.stats["pack_launches"] > 0 and out.stats["unpack_launches"] > 0
    assert costa.mx_items() > i0 and costa.scaled_items() == s0
    for r in range(P):
        assert_same(host(dc[r], tc), exp[r], tc, f"{kind} {op} rank {r}")
    if tc != F:
        merged = np.zeros(sc_shape, np.uint8)
        n_own = 0
        for r in range(P):
            own = mc.owned(c_case, P, r)
            first = (own if axis == ROWS else own.T)[::32, :]   # the rank owns a block with its first element
            mine = np.where(first, esc, 0).astype(np.uint8)
            SC[r].check(mine, f"{kind} {op} rank {r}: c_scales")
            merged = np.maximum(merged, mine)
            n_own += int(first.sum())
        assert n_own == esc.size and merged.tobytes() == esc.tobytes()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_fp6_loopback_exchange(mode):
    """PACK (a byte copy of the packed source) -> ncclSend/ncclRecv to self -> UNPACK on mx_kernel
    (tests/fp6_loopback_child.py)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fp6_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_, items = out[-1].split()
    assert int(n) == 3 and int(packs) > 0 and int(unpacks) > 0 and int(items) > 0, out[-1]
    assert (int(locals_) == 0) == (mode == "1"), out[-1]


# ------------------------------------------------------------------ refusals
@TYPES
def test_refusals_leave_everything_unchanged(costa, p):
    comm = costa.Comm.self(0)
    name = f6.TYPE_NAMES[p]
    other = E3M2 if p == E2M3 else E2M3
    a_case, c_case = f6.geometry("g204", "N")
    m, n = c_case.shape()
    ne = a_case.buf_elems(0, 1)
    sc0 = np.full((mc.n_blocks(m), n), 0x5A, np.uint8)
    dsa, dsc = dev(sc0), dev(sc0)
    SA = costa.mx_scales(dsa.view(mc.n_blocks(m), n), "rows")
    SC = costa.mx_scales(dsc.view(mc.n_blocks(m), n), "rows")
    c0 = np.resize(np.arange(251, dtype=np.uint8), ne * 16)
    da, dc = dev(np.resize(mc.quant_data(1, ne).view(np.uint8), ne * 16)), dev(c0)
    D, H, B, E4, I32, CF = costa.DOUBLE, costa.HALF, costa.BFLOAT16, costa.FP8_E4M3, costa.INT32, costa.CFLOAT
    FP4 = costa.FP4_E2M1
    CNAMES = dict(mc.fc.CNAMES)
    CNAMES.update({FP4: "FP4_E2M1", E2M3: "FP6_E2M3", E3M2: "FP6_E3M2"})

    def lay(case, code, buf):
        if code == F or code in FP6:
            return make_layout(costa, case, 0, buf.data_ptr(), 1, code)
        if code in (E4, costa.FP8_E5M2):
            return mc.make_layout(costa, case, 0, buf.data_ptr(), 1, code)
        return case.make_layout(0, buf.data_ptr(), 1, code)

    def untouched():
        assert dc.cpu().numpy().tobytes() == c0.tobytes()
        assert dsa.cpu().numpy().tobytes() == sc0.tobytes() and dsc.cpu().numpy().tobytes() == sc0.tobytes()

    def refused(call, match, *names):
        with pytest.raises(costa.CostaError, match=match) as e:
            call()
        assert e.value.code == 1, str(e.value)
        for nm in names:
            assert nm in str(e.value), str(e.value)
        untouched()

    A6, C6, Af, Cf = lay(a_case, p, da), lay(c_case, p, dc), lay(a_case, F, da), lay(c_case, F, dc)
    # transform_mx: FP6 with any other type is "no MX transform", naming both
    scaled_types = (E4, costa.FP8_E5M2, FP4, other)
    for code in (D, H, B, E4, costa.FP8_E5M2, FP4, other, I32, CF, costa.CDOUBLE):
        refused(lambda: costa.transform_mx(A6, lay(c_case, code, dc), comm, a_scales=SA,
                                           c_scales=SC if code in scaled_types else None),
                "no MX transform", name, CNAMES[code])
        refused(lambda: costa.transform_mx(lay(a_case, code, da), C6, comm, c_scales=SC,
                                           a_scales=SA if code in scaled_types else None),
                "no MX transform", name, CNAMES[code])
    # the descriptor rules hold for FP6 as for FP8
    refused(lambda: costa.transform_mx(Af, C6, comm, c_scales=SC, beta=2.0), "beta must be 0")
    refused(lambda: costa.transform_mx(A6, C6, comm, a_scales=SA, c_scales=SC, beta=-1.0), "beta must be 0")
    refused(lambda: costa.transform_mx(Af, C6, comm), "c_scales is required", name)
    refused(lambda: costa.transform_mx(Af, C6, comm, a_scales=SA, c_scales=SC), "a_scales given")
    refused(lambda: costa.transform_mx(A6, Cf, comm), "a_scales is required", name)
    refused(lambda: costa.transform_mx(A6, Cf, comm, a_scales=SA, c_scales=SC), "c_scales given")
    refused(lambda: costa.transform_mx(A6, C6, comm, c_scales=SC), "a_scales is required")
    refused(lambda: costa.transform_mx(A6, C6, comm, a_scales=SA), "c_scales is required")
    refused(lambda: costa.transform_mx(Af, C6, comm, c_scales=costa.MxScales(dsc.data_ptr(), ROWS, 1, 1)), "strides")
    refused(lambda: costa.transform_mx(A6, A6, comm, a_scales=SA, c_scales=SC), "in-place")
    # a tile boundary inside an MX block of C (64 x 96 blocks of A are fine, 40 x 24 are not)
    from casegen import BC
    refused(lambda: costa.transform_mx(lay(BC(204, 156, 40, 24), F, da), C6, comm, c_scales=SC), "MX block")
    # the quad rule: the other layout cuts C's packed rows at 66
    from casegen import Custom
    off = Custom([0, 66, m], [0, 32, n], [[0, 0], [0, 0]], ord="C", ld_pad=1)
    refused(lambda: costa.transform_mx(lay(off, F, da), C6, comm, c_scales=SC), "FP6 quad", name, "[0, 66)")
    refused(lambda: costa.transform_mx(A6, lay(off, F, dc), comm, a_scales=SA), "FP6 quad", name, "[64, 66)")
    # a host-resident FP6 layout
    ha, hc = np.zeros(ne * 3 // 4, np.uint8), np.zeros(ne * 4, np.uint8)
    refused(lambda: costa.transform_mx(make_layout(costa, a_case, 0, ha.ctypes.data, 1, p), Cf, comm, a_scales=SA),
            "device-resident")
    refused(lambda: costa.transform_mx(Af, make_layout(costa, c_case, 0, hc.ctypes.data, 1, p), comm, c_scales=SC),
            "device-resident")
    assert not hc.any()
    # every other entry point refuses the type by name
    rs = torch.ones(m, dtype=torch.float32, device="cuda")
    ra = torch.zeros(m, dtype=torch.float32, device="cuda")
    for A, Cl in ((A6, C6), (A6, Cf), (Af, C6)):
        refused(lambda: costa.transform(A, Cl, comm), name)
        refused(lambda: costa.transform_async(A, Cl, comm), name)
        refused(lambda: costa.transform_batch([A, A], [Cl, Cl], comm), name)
        refused(lambda: costa.transform_scaled(A, Cl, comm, row_scale=rs), name)
        refused(lambda: costa.transform_amax(A, Cl, comm, row_amax=ra), name)
        refused(lambda: costa.transform_tri(A, Cl, comm, "N", "U", 0), name)
    refused(lambda: costa.layout_amax(A6, comm, row_amax=ra), name)
    assert not ra.cpu().numpy().any()
    refused(lambda: costa.copy_and_transform(p, 8, 8, da.data_ptr(), 8, True, dc.data_ptr(), 8, True), name)
    top = np.zeros(1, costa.TILE_OP_DTYPE)
    top[0] = (0, 0, 8, 8, 8, 8, ALPHA << 4, 0)
    refused(lambda: costa.execute_tiles(p, top, [1, 0], da.data_ptr(), dc.data_ptr()), name)
    sop = np.zeros(1, costa.SCALED_OP_DTYPE)
    sop[0] = ((0, 0, 32, 8, 32, 32, ALPHA << 4 | F_ROWS, 0), 0, 0)
    for ta, tc in ((p, p), (F, p), (p, F)):
        refused(lambda: costa.execute_tiles_scaled(ta, tc, sop, [1, 0], da.data_ptr(), dc.data_ptr(), row_scale=rs),
                name)
    # tile lists: pairs, descriptors and the per-op half of the quad rule
    for code in (E4, FP4, other):
        refused(lambda: costa.execute_tiles_mx(p, code, sop, [1, 0], 64, 8, da.data_ptr(), dc.data_ptr(), a_scales=SA,
                                               c_scales=SC), "no MX kernel", name, CNAMES[code])
    refused(lambda: costa.execute_tiles_mx(F, p, sop, [1, 0], 64, 8, da.data_ptr(), dc.data_ptr()), "scale tensor")
    bad = sop.copy()
    bad["op"]["nf"] = 28                        # (ends at the edge of a 28-row matrix: no MX block is split)
    bad["op"]["ns"] = 6                         # 6 elements along s are fine for a copy-mode destination...
    costa.mx_check_ops(bad, ROWS, 28, 6)
    bad["op"]["flags"] |= TR                    # ...and split a group of a transpose-mode one
    refused(lambda: costa.execute_tiles_mx(F, p, bad, [1, 0], 28, 6, da.data_ptr(), dc.data_ptr(), c_scales=SC),
            "FP6 quad", name)
    bad = sop.copy()
    bad["op"]["nf"] = 30
    refused(lambda: costa.execute_tiles_mx(F, p, bad, [1, 0], 30, 8, da.data_ptr(), dc.data_ptr(), c_scales=SC),
            "FP6 quad", name)
    bad = sop.copy()
    bad["op"]["ldd"] = 34
    refused(lambda: costa.execute_tiles_mx(F, p, bad, [1, 0], 32, 8, da.data_ptr(), dc.data_ptr(), c_scales=SC),
            "FP6 quad", name)
    bad = sop.copy()
    bad["op"]["lds"] = 34
    refused(lambda: costa.execute_tiles_mx(p, F, bad, [1, 0], 32, 8, da.data_ptr(), dc.data_ptr(), a_scales=SA),
            "FP6 quad", name)
    # and the calls work afterwards
    _xf(costa, p, "quantise", "g204", "N", comm=comm)


# ------------------------------------------------------------------ neighbours
def test_fp4_fp8_and_plain_transforms_are_unchanged_around_fp6_calls(costa):
    """an FP8 and an FP4 transform_mx call and an ordinary transform of the same geometry give, before
    and after FP6 calls, the bytes they give alone: separate plans, no shared state"""
    import fp4_common as f4
    a_case, c_case = f6.geometry("g204", "T")
    m, n = c_case.shape()
    comm = costa.Comm.self(0)
    a = mc.quant_data(0x61, a_case.buf_elems(0, 1))
    nc = c_case.buf_elems(0, 1)
    c8, c4, cf = mc.fc.gen(mc.E4M3, 0x62, nc), f4.fp4_data(0x64, nc), mc.fc.gen(F, 0x63, nc)
    da, d8, d4, df = dev(a), dev(c8), dev(c4), dev(cf)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, F)
    C8 = mc.make_layout(costa, c_case, 0, d8.data_ptr(), 1, mc.E4M3)
    C4 = f4.make_layout(costa, c_case, 0, d4.data_ptr(), 1, f4.FP4)
    Cf = make_layout(costa, c_case, 0, df.data_ptr(), 1, F)

    def others():
        d8.copy_(dev(c8))
        d4.copy_(dev(c4))
        df.copy_(dev(cf))
        S8 = _scales_for(costa, (m, n), COLS, "block")
        S4 = _scales_for(costa, (m, n), COLS, "block")
        costa.transform_mx(A, C8, comm, "T", 0.75, 0.0, c_scales=S8.desc)
        costa.transform_mx(A, C4, comm, "T", 0.75, 0.0, c_scales=S4.desc)
        costa.transform(A, Cf, comm, "T", 0.75, 0.0)
        return (d8.cpu().numpy().tobytes(), S8.t.cpu().numpy().tobytes(), d4.cpu().numpy().tobytes(),
                S4.t.cpu().numpy().tobytes(), df.cpu().numpy().tobytes())
    before = others()
    exp8, _, _ = mc.expected_transform_mx(F, mc.E4M3, "T", 0.75, 0.0, a_case, c_case, 1, [a], [c8], c_axis=COLS)
    assert before[0] == exp8[0].tobytes()
    exp4, _, _ = f4.expected_transform_mx4(F, f4.FP4, "T", 0.75, 0.0, a_case, c_case, 1, [a], [c4], c_axis=COLS)
    assert before[2] == exp4[0].tobytes()
    ref = cf.copy()
    oracle.transform(oracle.FLOAT, "T", 0.75, 0.0, a_case.geom(1), [a], c_case.geom(1), [ref])
    assert before[4] == ref.tobytes()
    st0 = costa.get_stats()
    i0, s0 = costa.mx_items(), costa.scaled_items()
    _xf(costa, E2M3, "quantise", "g204", "T", c_axis=COLS, alpha=0.75, comm=comm)
    _xf(costa, E3M2, "requantise", "g204", "T", a_axis=ROWS, c_axis=COLS, alpha=ALPHA_RQ, comm=comm)
    st1 = costa.get_stats()
    assert st1["plan_misses"] - st0["plan_misses"] == 2      # the FP6 pairs have plans of their own
    assert costa.mx_items() > i0 and costa.scaled_items() == s0   # mx_items counts the FP6 sub-tiles
    assert others() == before
    assert costa.get_stats()["plan_misses"] == st1["plan_misses"]
