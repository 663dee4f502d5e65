"""MXFP4 on the GPU (costa_hip.h, "MXFP4"): the packed e2m1 instantiations of mx_kernel through
costa_hip_execute_tiles_mx, and costa_hip_transform_mx on one rank, on a stream, on emulated ranks and
through the loopback exchange.  Expected packed bytes and scale bytes come from the numpy model of
fp4_common.py; every comparison is exact and covers the whole destination buffer: neighbouring
nibbles, ld padding and the gaps between block buffers keep their fill."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fp4_common as f4
import mx_common as mc
import oracle
from emulated_ranks import drive
from fp4_common import CEIL, COLS, F, FLOOR, FP4, NAMES, ROWS, assert_same, make_layout
from test_gpu_mx import ScaleT, dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR, F_ROWS = 0x1, 0x80
BITCOPY, ALPHA, AXPBY = 0, 2, 3
NPT = {F: np.float32, FP4: np.uint8}
RND = {FLOOR: "floor", CEIL: "ceil"}
M, N = 202, 158          # 6 * 32 + 10 and 4 * 32 + 30: both = 2 mod 4
KINDS = {"quantise": (F, FP4), "dequantise": (FP4, F), "requantise": (FP4, FP4)}


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
    202 x 158 matrix.  Along the block axis (length L) every op starts on a multiple of 32 and ends on
    one or at the matrix edge, where the last MX block is partial: 10 of 32 rows, 30 of 32 columns.
    ld rules: 'v' a multiple of 32 (2-byte strips), 'b' 202 (= 2 mod 4: every other line starts on an
    odd byte, byte accesses); offset 2 puts the first element of a side on an odd byte."""
    L, O = (M, N) if axis == ROWS else (N, M)
    reg = [
        (0, 0, 64, 64, True, "v", "v", 0),          # one whole sub-tile, blocks along f (FULL path)
        (64, 0, 64, 64, False, "v", "v", 0),        # one whole sub-tile, blocks along s (FULL path)
        (128, 0, L - 128, 46, True, "b", "v", 0),   # up to the edge along f: a strip of 2, a partial block
        (128, 46, L - 128, 30, False, "v", "b", 0),  # the same with the blocks along s; 30 = 7 strips + 2
        (0, 64, 96, O - 64, True, "b", "b", 0),     # 96 x 94 (138): remainder sub-tiles on both sides
        (96, 64, 32, 18, False, "v", "v", 2),       # aligned ld, first element on an odd byte
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
    for k, (r0, c0, nr, nc, frow, sl, dl, off) in enumerate(regions):
        nf, ns = (nr, nc) if frow else (nc, nr)

        def place(at, fast, slow, rule, off):
            ld = (fast + 31) // 32 * 32 if rule == "v" else 202
            assert ld >= fast and ld % 2 == 0
            return at + off, ld, (at + off + ld * slow + 31) // 32 * 32
        s0, lds, src_at = place(src_at, nf, ns, sl, off)
        df, dslow = (ns, nf) if transpose else (nf, ns)
        d0, ldd, dst_at = place(dst_at, df, dslow, dl, off)
        flags = (TR if transpose else 0) | kind << 4 | slot << 16 | (F_ROWS if frow else 0)
        ops[k] = ((s0, d0, nf, ns, lds, ldd, flags, 0), r0, c0)
    return ops, src_at + 32, dst_at + 32


def _subtiles(ops):
    return sum(-(-int(o["op"]["nf"]) // 64) * -(-int(o["op"]["ns"]) // 64) for o in ops)


def _gpu_ops(ops, ta, tc):
    """element offsets -> byte offsets (4 per fp32 element, half a byte per FP4 element)"""
    g = ops.copy()
    for side, code in (("src", ta), ("dst", tc)):
        assert code == F or (ops["op"][side] % 2 == 0).all()
        g["op"][side] = ops["op"][side] * 4 if code == F else ops["op"][side] // 2
    return g


def _run_tiles(costa, ta, tc, ops, n_src, n_dst, m, n, alpha, beta, a_axis, c_axis, order, rounding, a_tr, what,
               src=None, sa=None):
    scal = np.array([alpha, beta], np.float32)
    if src is None:
        src = mc.quant_data(0xA1, n_src) if ta == F else f4.fp4_data(0xA2, n_src)
    dst0 = f4.fill(tc, 0xC1, n_dst)
    SA = SC = None
    if ta != F:
        am, an = (n, m) if a_tr else (m, n)
        shape = (mc.n_blocks(am), an) if a_axis == ROWS else (mc.n_blocks(an), am)
        SA = ScaleT(costa, a_axis, *shape, order, init=mc.scale_bytes(0x5A, shape) if sa is None else sa)
    if tc != F:
        shape = (mc.n_blocks(m), n) if c_axis == ROWS else (mc.n_blocks(n), m)
        SC = ScaleT(costa, c_axis, *shape, order)
    exp, esc, t = f4.expected_tiles_mx4(ta, tc, ops, alpha, beta, src, dst0, m, n, sa=SA.init if SA else None,
                                        a_axis=a_axis, a_transposed=a_tr, c_axis=c_axis if SC else None,
                                        rounding=rounding, sc_fill=SC.init if SC else None)
    ds, dd = dev(src), dev(dst0)
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


def _check_saturation(exp, t, rounding, what):
    codes = f4.unpack(exp)
    if rounding == FLOOR:  # the clamp ran: values above 6 before it, the saturating code stored
        assert (np.abs(t) > 6.0).any(), what
        assert ((codes & 7) == 7).any(), what
    else:
        assert (np.abs(t) <= 6.0).all(), what


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("order", ["block", "line"])
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_quantise_tile_lists(costa, transpose, axis, order, rounding):
    what = f"quantise f32->e2m1 {'tr' if transpose else 'copy'} axis {axis} {order} {RND[rounding]}"
    kind, alpha = (ALPHA, -0.5) if transpose or rounding == CEIL else (BITCOPY, 1.0)
    lst = _tile_list(costa, axis, transpose, kind)
    got, exp, esc, t = _run_tiles(costa, F, FP4, *lst, M, N, alpha, 0.0, None, axis, order, rounding, False, what)
    _check_saturation(exp, t, rounding, what)


@pytest.mark.parametrize("order", ["block", "line"])
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("a_tr", [False, True], ids=["a", "at"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_dequantise_tile_lists(costa, transpose, a_tr, axis, order):
    """beta != 0: the old destination values are read; a_scales indexed by A's matrix, also turned round"""
    what = f"dequantise e2m1->f32 {'tr' if transpose else 'copy'} a_tr {a_tr} axis {axis} {order}"
    lst = _tile_list(costa, ROWS if transpose else COLS, transpose, AXPBY)
    got, exp, _, _ = _run_tiles(costa, FP4, F, *lst, M, N, -0.5, 2.0, axis, None, order, FLOOR, a_tr, what)
    assert np.isfinite(exp).all()


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("axes", [(ROWS, COLS), (COLS, ROWS), (ROWS, ROWS), (COLS, COLS)],
                         ids=["rows-cols", "cols-rows", "rows-rows", "cols-cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_requantise_tile_lists(costa, transpose, axes, rounding):
    """alpha = 0.625 turns the source magnitudes 6 * 2^k into 1.875 * 2^(k+1): above 6 after the floor
    rule's scaling, so the clamp runs (a power of two times an e2m1 value alone never lands in (6, 8))"""
    a_axis, c_axis = axes
    what = f"requantise e2m1 {'tr' if transpose else 'copy'} axes {axes} {RND[rounding]}"
    order = "block" if rounding == FLOOR else "line"
    lst = _tile_list(costa, c_axis, transpose, ALPHA)
    got, exp, esc, t = _run_tiles(costa, FP4, FP4, *lst, M, N, 0.625, 0.0, a_axis, c_axis, order, rounding, transpose,
                                  what)
    _check_saturation(exp, t, rounding, what)


# ------------------------------------------------------------------ specials
TIE_VALUES = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)


def _special_blocks():
    """one block per column of a 32 x 8 matrix (blocks along rows)"""
    V = np.zeros((32, 8), np.float32)
    V[[2, 11, 30], 0] = -0.0                                           # all zero, some -0
    V[:, 1] = -0.5
    V[9, 1] = np.inf                                                   # an inf
    V[:, 2] = 0.25
    V[9, 2] = np.nan                                                   # a NaN
    V[:, 3] = np.float32(2.0 ** -127) * np.linspace(-1, 1, 32, dtype=np.float32)   # maximum below 2^-125
    V[:, 4] = np.float32(2.5e38) * np.linspace(-1, 1, 32, dtype=np.float32)        # maximum near 2^127
    V[:, 5] = np.linspace(-40, 40, 32, dtype=np.float32)
    V[5, 5] = 48.0                                                     # scales to exactly 6.0
    V[:, 6] = V[:, 5]
    V[5, 6] = np.nextafter(np.float32(48.0), np.float32(64.0))         # just above: ceil raises E, floor saturates
    V[:14, 7] = np.concatenate([TIE_VALUES, -TIE_VALUES]) * np.float32(2.0 ** -4)  # the seven ties at one scale
    return V


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("frow", [True, False], ids=["along-f", "along-s"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_special_blocks(costa, transpose, frow, rounding):
    V = _special_blocks()
    m, n = V.shape
    src = (V.T if frow else V).reshape(-1).copy()  # element (f, s) at s * lds + f
    nf, ns = (m, n) if frow else (n, m)
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ldd = ns if transpose else nf
    ops[0] = ((0, 0, nf, ns, nf, ldd, (TR if transpose else 0) | BITCOPY << 4 | (F_ROWS if frow else 0), 0), 0, 0)
    what = f"specials e2m1 {'tr' if transpose else 'copy'} frow {frow} {RND[rounding]}"
    got, exp, esc, t = _run_tiles(costa, F, FP4, ops, src.size, m * n, m, n, 1.0, 0.0, None, ROWS, "block", rounding,
                                  False, what, src=src)
    E = esc[0]
    assert E[0] == 0 and E[1] == 255 and E[2] == 255 and E[3] == 0 and E[4] == 254 - 2
    assert E[5] == 127 + 5 - 2 and E[6] == 127 + 5 - 2 + (1 if rounding == CEIL else 0) and E[7] == 127 - 4
    # the codes of the target matrix, whatever the destination's orientation
    codes = f4.unpack(got).reshape((m, n) if transpose == frow else (n, m))
    Q = codes if transpose == frow else codes.T
    assert (Q[:, 1] == 0).all() and (Q[:, 2] == 0).all()               # E = 255: code 0x0 everywhere
    assert list(Q[[2, 11, 30], 0]) == [8, 8, 8] and (np.delete(Q[:, 0], [2, 11, 30]) == 0).all()
    assert Q[5, 5] == 0x7 and Q[5, 6] == (0x7 if rounding == FLOOR else 0x5)
    assert list(Q[:14, 7]) == [0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14]


# ------------------------------------------------------------------ exhaustive dequantise
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_every_byte_against_the_special_scale_bytes(costa, transpose, axis):
    """all 256 byte values (every pair of codes) times the bytes 0, 1, 126, 127, 128, 254, 255:
    subnormal products are kept, 255 makes NaNs, -0 keeps its sign.  The source is 56 lines of 64
    elements with the blocks along the lines (f): line s holds the 32 byte values 32 * (s % 8) .. + 31
    and meets the scale byte number s % 7, so the 56 lines give every (byte value, scale byte) pair."""
    nf, ns = 64, 56
    vals = np.array([0, 1, 126, 127, 128, 254, 255], np.uint8)
    frow = axis == ROWS                        # the blocks run along f: f walks rows for ROWS, columns for COLS
    m, n = (nf, ns) if frow else (ns, nf)
    sa = np.broadcast_to(vals[np.arange(ns) % 7][None, :], (2, ns)).copy()      # [block, line]
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, nf, ns, nf, ns if transpose else nf, (TR if transpose else 0) | ALPHA << 4 | (F_ROWS if frow else 0),
               0), 0, 0)
    src = np.resize(np.arange(256, dtype=np.uint8), nf * ns // 2)
    f, s_ = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
    met = src[(s_ * nf + f) // 2].astype(np.int64) * 256 + sa[f // 32, s_]
    assert np.unique(met).size == 256 * vals.size
    what = f"every byte e2m1 {'tr' if transpose else 'copy'} axis {axis}"
    got, exp, _, _ = _run_tiles(costa, FP4, F, ops, nf * ns, nf * ns, m, n, 1.0, 0.0, axis, None, "line", FLOOR, False,
                                what, src=src, sa=sa)
    sub = exp[(exp != 0) & np.isfinite(exp) & (np.abs(exp) < 2.0 ** -126)]
    assert sub.size > 0 and np.isnan(exp).any() and (np.signbit(exp) & (exp == 0)).any()


# ------------------------------------------------------------------ transform_mx on one rank
def _scales_for(costa, case_shape, axis, order, init=None, fill=0xA5):
    rows, cols = case_shape
    shape = (mc.n_blocks(rows), cols) if axis == ROWS else (mc.n_blocks(cols), rows)
    return ScaleT(costa, axis, *shape, order, init=None if init is None else init(shape), fill=fill)


def _xf(costa, kind, geom, op, a_axis=ROWS, c_axis=ROWS, rounding=FLOOR, alpha=1.0, beta=0.0, order="block",
        stream=None, comm=None):
    """one one-rank transform_mx against the model -> t before the clamp"""
    ta, tc = KINDS[kind]
    a_case, c_case = f4.geometry(geom, op)
    what = f"{kind} {NAMES[ta]}->{NAMES[tc]} {geom} {op}"
    na, nc = a_case.buf_elems(0, 1), c_case.buf_elems(0, 1)
    a = mc.quant_data(0x31, na) if ta == F else f4.fp4_data(0x32, na)
    c = f4.fill(tc, 0x33, nc)
    SA = _scales_for(costa, a_case.shape(), a_axis, order, lambda s: mc.scale_bytes(0x34, s)) if ta != F else None
    SC = _scales_for(costa, c_case.shape(), c_axis, order) if tc != F else None
    exp, esc, t = f4.expected_transform_mx4(ta, tc, op, alpha, beta, a_case, c_case, 1, [a], [c],
                                            sa=SA.init if SA else None, a_axis=a_axis,
                                            c_axis=c_axis if SC else None, rounding=rounding)
    da, dc = dev(a), dev(c)
    assert da.numel() == f4.buf_bytes(ta, na) and dc.numel() == f4.buf_bytes(tc, nc)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    comm = comm or costa.Comm.self(0)
    i0 = costa.mx_items()
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
    assert costa.mx_items() > i0
    return t


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["g202", "g202pad", "custom32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_transform_mx_one_rank(costa, kind, geom, op):
    rounding = CEIL if geom == "g202pad" else FLOOR
    # requantise 'T' turns the block axis round ('N' keeps it); the others alternate with the geometry
    a_axis = ROWS if geom in ("g202", "custom32") else COLS
    c_axis = (COLS if a_axis == ROWS else ROWS) if kind == "requantise" and op == "T" else a_axis
    alpha, beta = (-0.5, 2.0) if kind == "dequantise" and op == "T" else (1.0, 0.0) if op == "N" else (0.625, 0.0)
    t = _xf(costa, kind, geom, op, a_axis, c_axis, rounding, alpha, beta, order="block" if op == "N" else "line")
    if kind == "quantise" and rounding == FLOOR:
        assert (np.abs(t) > 6.0).any()


def test_requantise_transposed_keeps_cols_blocks(costa):
    """'T' from axis COLS of A to axis COLS of the transposed matrix: no byte-wise transpose can do it,
    the model dequantises and requantises"""
    _xf(costa, "requantise", "g202", "T", a_axis=COLS, c_axis=COLS, alpha=0.625)


def test_transform_mx_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _xf(costa, "quantise", "g202", "T", c_axis=COLS, alpha=0.75, stream=s)


# ------------------------------------------------------------------ several ranks on one GPU
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", ["quantise", "dequantise"])
def test_emulated_ranks_2x2(costa, kind, op):
    """quantise sends fp32 packages, dequantise packed FP4 packages counted in bytes; each rank's c_scales
    holds exactly its own blocks' bytes over a zero fill and their maximum is the model's tensor"""
    P = 4
    ta, tc = KINDS[kind]
    a_case, c_case = f4.geometry("g202", op, (2, 2))
    m, n = c_case.shape()
    alpha, beta = (0.75, 0.0) if kind == "quantise" else (-0.5, 2.0)
    a = [mc.quant_data(0x40 + r, a_case.buf_elems(r, P)) if ta == F else f4.fp4_data(0x40 + r, a_case.buf_elems(r, P))
         for r in range(P)]
    c = [f4.fill(tc, 0x50 + r, c_case.buf_elems(r, P)) for r in range(P)]
    axis = COLS if op == "T" else ROWS
    am, an = a_case.shape()
    sa_shape = (mc.n_blocks(am), an) if axis == ROWS else (mc.n_blocks(an), am)
    sc_shape = (mc.n_blocks(m), n) if axis == ROWS else (mc.n_blocks(n), m)
    sa = mc.scale_bytes(0x66, sa_shape) if ta != F else None
    exp, esc, _ = f4.expected_transform_mx4(ta, tc, op, alpha, beta, a_case, c_case, P, a, c, sa=sa, a_axis=axis,
                                            c_axis=axis if tc != F else None)
    da, dc = [dev(x) for x in a], [dev(x) for x in c]
    lay = [(make_layout(costa, a_case, r, da[r].data_ptr(), P, ta), make_layout(costa, c_case, r, dc[r].data_ptr(), P, tc))
           for r in range(P)]
    plans = [costa.plan_export_scaled(lay[r][0], lay[r][1], r, P, op, alpha, beta) for r in range(P)]
    assert all(p.send_elems > 0 and p.recv_elems > 0 for p in plans)
    SA = [ScaleT(costa, axis, *sa_shape, "line", init=sa) if ta != F else None for r in range(P)]
    SC = [ScaleT(costa, axis, *sc_shape, "block", fill=0) if tc != F else None for r in range(P)]
    i0, s0 = costa.mx_items(), costa.scaled_items()

    def call(r, comm):
        costa.transform_mx(lay[r][0], lay[r][1], comm, op, alpha, beta, a_scales=SA[r].desc if SA[r] else None,
                           c_scales=SC[r].desc if SC[r] else None)

    # bytes of a package unit: an fp32 element, or one byte (two elements) of a packed package
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
def test_fp4_loopback_exchange(mode):
    """PACK (a byte copy of the packed source) -> ncclSend/ncclRecv to self -> UNPACK on mx_kernel
    (tests/fp4_loopback_child.py)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fp4_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_, items = out[-1].split()
    assert int(n) == 3 and int(packs) > 0 and int(unpacks) > 0 and int(items) > 0, out[-1]
    assert (int(locals_) == 0) == (mode == "1"), out[-1]


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_unchanged(costa):
    comm = costa.Comm.self(0)
    a_case, c_case = f4.geometry("g202", "N")
    m, n = c_case.shape()
    ne = a_case.buf_elems(0, 1)
    sc0 = np.full((mc.n_blocks(m), n), 0x5A, np.uint8)
    dsa, dsc = dev(sc0), dev(sc0)
    SA = costa.mx_scales(dsa.view(mc.n_blocks(m), n), "rows")
    SC = costa.mx_scales(dsc.view(mc.n_blocks(m), n), "rows")
    c0 = np.resize(np.arange(251, dtype=np.uint8), ne * 16)
    da, dc = dev(np.resize(mc.quant_data(1, ne).view(np.uint8), ne * 16)), dev(c0)
    D, H, B, E4, I32, CF = costa.DOUBLE, costa.HALF, costa.BFLOAT16, costa.FP8_E4M3, costa.INT32, costa.CFLOAT

    def lay(case, code, buf):
        if code in (F, FP4):
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

    A4, C4, Af, Cf = lay(a_case, FP4, da), lay(c_case, FP4, dc), lay(a_case, F, da), lay(c_case, F, dc)
    # transform_mx: FP4 with any other type is "no MX transform", naming both
    for code in (D, H, B, E4, costa.FP8_E5M2, I32, CF, costa.CDOUBLE):
        name = mc.fc.CNAMES[code]
        refused(lambda: costa.transform_mx(A4, lay(c_case, code, dc), comm, a_scales=SA,
                                           c_scales=SC if code in (E4, costa.FP8_E5M2) else None),
                "no MX transform", "FP4_E2M1", name)
        refused(lambda: costa.transform_mx(lay(a_case, code, da), C4, comm, c_scales=SC,
                                           a_scales=SA if code in (E4, costa.FP8_E5M2) else None),
                "no MX transform", "FP4_E2M1", name)
    # the descriptor rules hold for FP4 as for FP8
    refused(lambda: costa.transform_mx(Af, C4, comm, c_scales=SC, beta=2.0), "beta must be 0")
    refused(lambda: costa.transform_mx(A4, C4, comm, a_scales=SA, c_scales=SC, beta=-1.0), "beta must be 0")
    refused(lambda: costa.transform_mx(Af, C4, comm), "c_scales is required", "FP4_E2M1")
    refused(lambda: costa.transform_mx(Af, C4, comm, a_scales=SA, c_scales=SC), "a_scales given")
    refused(lambda: costa.transform_mx(A4, Cf, comm), "a_scales is required", "FP4_E2M1")
    refused(lambda: costa.transform_mx(A4, Cf, comm, a_scales=SA, c_scales=SC), "c_scales given")
    refused(lambda: costa.transform_mx(A4, C4, comm, c_scales=SC), "a_scales is required")
    refused(lambda: costa.transform_mx(A4, C4, comm, a_scales=SA), "c_scales is required")
    refused(lambda: costa.transform_mx(Af, C4, comm, c_scales=costa.MxScales(dsc.data_ptr(), ROWS, 1, 1)), "strides")
    refused(lambda: costa.transform_mx(A4, A4, comm, a_scales=SA, c_scales=SC), "in-place")
    # a tile boundary inside an MX block of C (64 x 96 blocks of A are fine, 40 x 24 are not)
    from casegen import BC
    refused(lambda: costa.transform_mx(lay(BC(202, 158, 40, 24), F, da), C4, comm, c_scales=SC), "MX block")
    # the evenness rule: the other layout cuts C's packed rows at 65
    from casegen import Custom
    odd = Custom([0, 65, m], [0, 32, n], [[0, 0], [0, 0]], ord="C", ld_pad=1)
    refused(lambda: costa.transform_mx(lay(odd, F, da), C4, comm, c_scales=SC), "FP4 pair", "[0, 65)")
    refused(lambda: costa.transform_mx(A4, lay(odd, F, dc), comm, a_scales=SA), "FP4 pair", "[64, 65)")
    # a host-resident FP4 layout
    ha, hc = np.zeros(ne // 2, np.uint8), np.zeros(ne * 4, np.uint8)
    refused(lambda: costa.transform_mx(make_layout(costa, a_case, 0, ha.ctypes.data, 1, FP4), Cf, comm, a_scales=SA),
            "device-resident")
    refused(lambda: costa.transform_mx(Af, make_layout(costa, c_case, 0, hc.ctypes.data, 1, FP4), comm, c_scales=SC),
            "device-resident")
    assert not hc.any()
    # every other entry point refuses the type by name
    rs = torch.ones(m, dtype=torch.float32, device="cuda")
    ra = torch.zeros(m, dtype=torch.float32, device="cuda")
    for A, Cl in ((A4, C4), (A4, Cf), (Af, C4)):
        refused(lambda: costa.transform(A, Cl, comm), "FP4_E2M1")
        refused(lambda: costa.transform_async(A, Cl, comm), "FP4_E2M1")
        refused(lambda: costa.transform_batch([A, A], [Cl, Cl], comm), "FP4_E2M1")
        refused(lambda: costa.transform_scaled(A, Cl, comm, row_scale=rs), "FP4_E2M1")
        refused(lambda: costa.transform_amax(A, Cl, comm, row_amax=ra), "FP4_E2M1")
        refused(lambda: costa.transform_tri(A, Cl, comm, "N", "U", 0), "FP4_E2M1")
    refused(lambda: costa.layout_amax(A4, comm, row_amax=ra), "FP4_E2M1")
    assert not ra.cpu().numpy().any()
    refused(lambda: costa.copy_and_transform(FP4, 8, 8, da.data_ptr(), 8, True, dc.data_ptr(), 8, True), "FP4_E2M1")
    top = np.zeros(1, costa.TILE_OP_DTYPE)
    top[0] = (0, 0, 8, 8, 8, 8, ALPHA << 4, 0)
    refused(lambda: costa.execute_tiles(FP4, top, [1, 0], da.data_ptr(), dc.data_ptr()), "FP4_E2M1")
    sop = np.zeros(1, costa.SCALED_OP_DTYPE)
    sop[0] = ((0, 0, 32, 8, 32, 32, ALPHA << 4 | F_ROWS, 0), 0, 0)
    for ta, tc in ((FP4, FP4), (F, FP4), (FP4, F)):
        refused(lambda: costa.execute_tiles_scaled(ta, tc, sop, [1, 0], da.data_ptr(), dc.data_ptr(), row_scale=rs),
                "FP4_E2M1")
    # tile lists: pairs, descriptors and the per-op half of the evenness rule
    refused(lambda: costa.execute_tiles_mx(FP4, E4, sop, [1, 0], 64, 8, da.data_ptr(), dc.data_ptr(), a_scales=SA,
                                           c_scales=SC), "no MX kernel", "FP4_E2M1", "FP8_E4M3")
    refused(lambda: costa.execute_tiles_mx(F, FP4, sop, [1, 0], 64, 8, da.data_ptr(), dc.data_ptr()), "scale tensor")
    bad = sop.copy()
    bad["op"]["nf"] = 30                        # (ends at the edge of a 30-row matrix: no MX block is split)
    bad["op"]["ns"] = 7                         # 7 elements along s are fine for a copy-mode destination...
    costa.mx_check_ops(bad, ROWS, 30, 7)
    bad["op"]["flags"] |= TR                    # ...and split a byte of a transpose-mode one
    refused(lambda: costa.execute_tiles_mx(F, FP4, bad, [1, 0], 30, 7, da.data_ptr(), dc.data_ptr(), c_scales=SC),
            "FP4 pair")
    bad = sop.copy()
    bad["op"]["nf"] = 31
    refused(lambda: costa.execute_tiles_mx(F, FP4, bad, [1, 0], 31, 8, da.data_ptr(), dc.data_ptr(), c_scales=SC),
            "FP4 pair")
    bad = sop.copy()
    bad["op"]["ldd"] = 33
    refused(lambda: costa.execute_tiles_mx(F, FP4, bad, [1, 0], 32, 8, da.data_ptr(), dc.data_ptr(), c_scales=SC),
            "FP4 pair")
    bad = sop.copy()
    bad["op"]["lds"] = 33
    refused(lambda: costa.execute_tiles_mx(FP4, F, bad, [1, 0], 32, 8, da.data_ptr(), dc.data_ptr(), a_scales=SA),
            "FP4 pair")
    # and the calls work afterwards
    _xf(costa, "quantise", "g202", "N", comm=comm)


# ------------------------------------------------------------------ neighbours
def test_fp8_and_plain_transforms_are_unchanged_around_an_fp4_call(costa):
    """an FP8 transform_mx call and an ordinary transform of the same geometry give, before and after an
    FP4 call, the bytes they give alone: separate plans, no shared state"""
    a_case, c_case = f4.geometry("g202", "T")
    m, n = c_case.shape()
    comm = costa.Comm.self(0)
    a = mc.quant_data(0x61, a_case.buf_elems(0, 1))
    nc = c_case.buf_elems(0, 1)
    c8, cf = mc.fc.gen(mc.E4M3, 0x62, nc), mc.fc.gen(F, 0x63, nc)
    da, d8, df = dev(a), dev(c8), dev(cf)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, F)
    C8 = mc.make_layout(costa, c_case, 0, d8.data_ptr(), 1, mc.E4M3)
    Cf = make_layout(costa, c_case, 0, df.data_ptr(), 1, F)

    def others():
        d8.copy_(dev(c8))
        df.copy_(dev(cf))
        S8 = _scales_for(costa, (m, n), COLS, "block")
        costa.transform_mx(A, C8, comm, "T", 0.75, 0.0, c_scales=S8.desc)
        costa.transform(A, Cf, comm, "T", 0.75, 0.0)
        return d8.cpu().numpy().tobytes(), S8.t.cpu().numpy().tobytes(), df.cpu().numpy().tobytes()
    before = others()
    exp8, esc8, _ = mc.expected_transform_mx(F, mc.E4M3, "T", 0.75, 0.0, a_case, c_case, 1, [a], [c8], c_axis=COLS)
    assert before[0] == exp8[0].tobytes()
    ref = cf.copy()
    oracle.transform(oracle.FLOAT, "T", 0.75, 0.0, a_case.geom(1), [a], c_case.geom(1), [ref])
    assert before[2] == ref.tobytes()
    st0 = costa.get_stats()
    _xf(costa, "quantise", "g202", "T", c_axis=COLS, alpha=0.75, comm=comm)
    _xf(costa, "requantise", "g202", "T", a_axis=ROWS, c_axis=COLS, alpha=0.625, comm=comm)
    st1 = costa.get_stats()
    assert st1["plan_misses"] - st0["plan_misses"] == 2      # the FP4 pairs have plans of their own
    assert others() == before
    assert costa.get_stats()["plan_misses"] == st1["plan_misses"]
