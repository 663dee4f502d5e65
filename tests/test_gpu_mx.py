"""MX block-scaled transforms on the GPU (costa_hip.h, "MX block-scaled transforms"): mx_kernel through
costa_hip_execute_tiles_mx, and costa_hip_transform_mx on one rank, on a stream, on emulated ranks and
through the loopback exchange.  Expected data bits and scale bytes come from the model of mx_common.py;
scale bytes are compared exactly, together with the bytes around them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mx_common as mc
import oracle
from emulated_ranks import drive
from mx_common import CEIL, COLS, E4M3, E5M2, F, FLOOR, NAMES, ROWS, assert_bits, make_layout

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR, F_ROWS = 0x1, 0x80
BITCOPY, ALPHA, AXPBY = 0, 2, 3
ESIZE = {F: 4, E4M3: 1, E5M2: 1}
NPT = {F: np.float32, E4M3: np.uint8, E5M2: np.uint8}
QS = [E4M3, E5M2]
RND = {FLOOR: "floor", CEIL: "ceil"}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def host(t, code):
    return t.cpu().numpy().view(NPT[code])


class ScaleT:
    """a scale tensor [block, line] inside a larger device buffer of fill bytes: block-major (lines
    consecutive, a gap of 3 bytes after each block row) or line-major (blocks consecutive, a gap of 2
    after each line), 32 sentinel bytes on each side"""
    PAD = 32

    def __init__(self, costa, axis, nb, lines, order, init=None, fill=0xA5):
        self.axis, self.nb, self.lines = axis, nb, lines
        if order == "block":
            self.bs, self.ls = lines + 3, 1
            size = nb * self.bs
        else:
            self.bs, self.ls = 1, nb + 2
            size = lines * self.ls
        self.at = (self.PAD + np.arange(nb)[:, None] * self.bs + np.arange(lines)[None, :] * self.ls).astype(np.int64)
        full = np.full(size + 2 * self.PAD, fill, np.uint8)
        self.init = np.full((nb, lines), fill, np.uint8) if init is None else np.asarray(init, np.uint8)
        full[self.at] = self.init
        self.full0 = full
        self.t = dev(full)
        self.desc = costa.MxScales(self.t.data_ptr() + self.PAD, axis, self.bs, self.ls)

    def check(self, exp, what):
        """the tensor holds `exp` exactly and every other byte of the buffer is unchanged"""
        got = self.t.cpu().numpy()
        want = self.full0.copy()
        want[self.at] = exp
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{what}: {bad.size} scale / surrounding bytes differ, first at buffer byte {bad[0]}: "
                               f"got {int(got[bad[0]])}, expected {int(want[bad[0]])}")


# ------------------------------------------------------------------ kernel level: tile lists
# target regions (row0, col0, rows, cols, F_ROWS, source shift, destination shift) for blocks along
# ROWS of a 205 x 120 matrix; several ops share block rows and columns of the scale tensor
REGIONS = [
    (0, 0, 64, 64, True, 0, 0),       # one whole sub-tile, blocks along f (FULL path)
    (96, 52, 64, 64, False, 0, 0),    # one whole sub-tile, blocks along s (FULL path)
    (64, 0, 96, 40, False, 0, 0),     # 96 x 40: partial sub-tiles
    (0, 64, 32, 1, True, 0, 0),       # 32 x 1
    (160, 3, 45, 21, True, 0, 0),     # ends at the matrix edge: 45 along the block axis, a block of 13
    (160, 30, 45, 9, False, 0, 0),    # the same with the blocks along s
    (32, 65, 64, 7, True, 1, 0),      # odd source offset (VEC_SRC clear)
    (96, 40, 64, 10, False, 0, 3),    # odd destination offset (VEC_DST clear)
]
M_ROWS, N_ROWS = 205, 120


def _tile_list(costa, axis, transpose, kind, slot):
    """-> (ops with ELEMENT offsets, source elements, destination elements, m, n)"""
    ops = np.zeros(len(REGIONS), costa.SCALED_OP_DTYPE)
    src_at = dst_at = 0
    for k, (r0, c0, nr, nc, frow, s_off, d_off) in enumerate(REGIONS):
        if axis == COLS:  # the same regions turned round: blocks along columns
            r0, c0, nr, nc, frow = c0, r0, nc, nr, not frow
        nf, ns = (nr, nc) if frow else (nc, nr)

        def place(at, fast, slow, off):
            ld = (fast + 15) // 16 * 16 + (1 if off else 0)
            return at + off, ld, (at + off + ld * slow + 15) // 16 * 16
        s0, lds, src_at = place(src_at, nf, ns, s_off)
        df, dslow = (ns, nf) if transpose else (nf, ns)
        d0, ldd, dst_at = place(dst_at, df, dslow, d_off)
        flags = (TR if transpose else 0) | kind << 4 | slot << 16 | (F_ROWS if frow else 0)
        ops[k] = ((s0, d0, nf, ns, lds, ldd, flags, 0), r0, c0)
    m, n = (M_ROWS, N_ROWS) if axis == ROWS else (N_ROWS, M_ROWS)
    return ops, src_at + 16, dst_at + 16, m, n


def _subtiles(ops):
    return sum(-(-int(o["op"]["nf"]) // 64) * -(-int(o["op"]["ns"]) // 64) for o in ops)


def _gpu_ops(ops, ta, tc):
    g = ops.copy()
    g["op"]["src"] = ops["op"]["src"] * ESIZE[ta]
    g["op"]["dst"] = ops["op"]["dst"] * ESIZE[tc]
    return g


def _fp8_data(tq, seed, n):
    return mc.cvt(mc.quant_data(seed, n), tq)


def _run_tiles(costa, ta, tc, ops, n_src, n_dst, m, n, alpha, beta, a_axis, c_axis, order, rounding, a_tr, what,
               src=None, sa=None):
    scal = np.array([alpha, beta], np.float32)
    if src is None:
        src = mc.quant_data(0xA1, n_src) if ta == F else _fp8_data(ta, 0xA2, n_src)
    dst0 = mc.fc.gen(tc, 0xC1, n_dst)
    SA = SC = None
    if ta != F:
        am, an = (n, m) if a_tr else (m, n)
        shape = (mc.n_blocks(am), an) if a_axis == ROWS else (mc.n_blocks(an), am)
        SA = ScaleT(costa, a_axis, *shape, order, init=mc.scale_bytes(0x5A, shape) if sa is None else sa)
    if tc != F:
        shape = (mc.n_blocks(m), n) if c_axis == ROWS else (mc.n_blocks(n), m)
        SC = ScaleT(costa, c_axis, *shape, order)
    exp, esc, t = mc.expected_tiles_mx(ta, tc, ops, alpha, beta, src, dst0, m, n, sa=SA.init if SA else None,
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
    assert_bits(got, exp, tc, what + ": destination")
    assert costa.mx_items() - i0 == _subtiles(ops)
    assert costa.scaled_items() == s0 and costa.amax_items() == a0
    assert ds.cpu().numpy().tobytes() == np.ascontiguousarray(src).tobytes()
    return got, exp, esc, t


def _check_saturation(tc, got, exp, t, rounding, what):
    fm = float(mc.FMAX[tc])
    mc.assert_data_finite(exp, tc, what)
    if rounding == FLOOR:  # the clamp ran: values above fmax before it, +-fmax stored
        assert (np.abs(t) > fm).any(), what
        assert (np.abs(mc.widen(got, tc)) == fm).any(), what
    else:
        assert (np.abs(t) <= fm).all(), what


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("order", ["block", "line"])
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_quantise_tile_lists(costa, transpose, axis, order, tq, rounding):
    what = f"quantise f32->{NAMES[tq]} {'tr' if transpose else 'copy'} axis {axis} {order} {RND[rounding]}"
    kind, alpha = (ALPHA, -0.5) if transpose or rounding == CEIL else (BITCOPY, 1.0)
    lst = _tile_list(costa, axis, transpose, kind, 0)
    got, exp, esc, t = _run_tiles(costa, F, tq, *lst, alpha, 0.0, None, axis, order, rounding, False, what)
    _check_saturation(tq, got, exp, t, rounding, what)


@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("order", ["block", "line"])
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("a_tr", [False, True], ids=["a", "at"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_dequantise_tile_lists(costa, transpose, a_tr, axis, order, tq):
    """beta != 0: the old destination values are read; a_scales indexed by A's matrix, also turned round"""
    what = f"dequantise {NAMES[tq]}->f32 {'tr' if transpose else 'copy'} a_tr {a_tr} axis {axis} {order}"
    lst = _tile_list(costa, ROWS if transpose else COLS, transpose, AXPBY, 0)
    got, exp, _, _ = _run_tiles(costa, tq, F, *lst, -0.5, 2.0, axis, None, order, FLOOR, a_tr, what)
    assert np.isfinite(exp).all()


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("axes", [(ROWS, COLS), (COLS, ROWS), (ROWS, ROWS), (COLS, COLS)],
                         ids=["rows-cols", "cols-rows", "rows-rows", "cols-cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_requantise_tile_lists(costa, transpose, axes, tq, rounding):
    a_axis, c_axis = axes
    what = f"requantise {NAMES[tq]} {'tr' if transpose else 'copy'} axes {axes} {RND[rounding]}"
    order = "block" if rounding == FLOOR else "line"
    lst = _tile_list(costa, c_axis, transpose, ALPHA, 0)
    got, exp, esc, t = _run_tiles(costa, tq, tq, *lst, 0.75, 0.0, a_axis, c_axis, order, rounding, transpose, what)
    _check_saturation(tq, got, exp, t, rounding, what)


# ------------------------------------------------------------------ specials
def _special_blocks(tq):
    """one block per column of a 32 x 10 matrix (blocks along rows)"""
    fmax = float(mc.FMAX[tq])
    V = np.zeros((32, 10), np.float32)
    # column 0: all zeros
    V[:, 1] = np.float32(1e-42) * np.arange(1, 33, dtype=np.float32)   # all subnormal
    V[:, 2] = 0.25
    V[9, 2] = np.nan                                                   # one NaN
    V[:, 3] = -0.5
    V[9, 3] = np.inf                                                   # one +inf
    V[:, 4] = np.linspace(-1, 1, 32, dtype=np.float32) * 2.0 ** -5
    V[3, 4] = 2.0 ** -5                                                # amax exactly 2^k
    V[:, 5] = np.linspace(-1, 1, 32, dtype=np.float32)
    V[5, 5] = fmax * 2.0 ** 4                                          # amax exactly fmax * 2^k
    V[:, 6] = np.linspace(0.1, 1.7, 32, dtype=np.float32)
    V[7, 6] = 1.9375                                                   # scales into (fmax, 2^(emax+1))
    V[2, 7] = -0.0                                                     # -0 in a zero block
    V[:, 8] = np.float32(2.5e38)                                       # the largest exponents
    V[:, 9] = np.float32(2.0 ** -126)                                  # the smallest normal
    return V


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("frow", [True, False], ids=["along-f", "along-s"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_special_blocks(costa, transpose, frow, tq, rounding):
    V = _special_blocks(tq)
    m, n = V.shape
    # blocks along rows; with frow the op's fast index walks rows, else the source holds V transposed
    src = (V.T if frow else V).reshape(-1).copy()  # element (f, s) at s * lds + f
    nf, ns = (m, n) if frow else (n, m)
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ldd = (ns if transpose else nf)
    ops[0] = ((0, 0, nf, ns, nf, ldd, (TR if transpose else 0) | BITCOPY << 4 | (F_ROWS if frow else 0), 0), 0, 0)
    what = f"specials {NAMES[tq]} {'tr' if transpose else 'copy'} frow {frow} {RND[rounding]}"
    got, exp, esc, t = _run_tiles(costa, F, tq, ops, src.size, m * n, m, n, 1.0, 0.0, None, ROWS, "block", rounding,
                                  False, what, src=src)
    emax = mc.EMAX[tq]
    E = esc[0]
    assert E[0] == 0 and E[1] == 0 and E[2] == 255 and E[3] == 255 and E[7] == 0
    assert E[4] == 127 - 5 - emax and E[8] == 254 - emax and E[9] == 0
    assert E[5] == 127 + 4                                             # fmax * 2^4 scales exactly onto fmax
    assert E[6] == 127 - emax + (1 if rounding == CEIL else 0)
    w = mc.widen(got, tq)
    assert np.isnan(w).sum() == 64                                     # the NaN and the inf block, nothing else


@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("axis", [ROWS, COLS], ids=["rows", "cols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_input_scale_bytes(costa, transpose, axis, tq):
    """dequantise with the bytes 0, 1, 127, 254 and 255: subnormal products are kept, 255 is a NaN"""
    m, n = 64, 40
    shape = (mc.n_blocks(m), n) if axis == ROWS else (mc.n_blocks(n), m)
    sa = np.resize(np.array([0, 1, 127, 254, 255, 127, 1], np.uint8), shape[0] * shape[1]).reshape(shape)
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, m, n, m, n if transpose else m, (TR if transpose else 0) | ALPHA << 4 | F_ROWS, 0), 0, 0)
    src = np.resize(np.arange(256, dtype=np.uint8), m * n)  # every bit pattern of the type
    what = f"scale bytes {NAMES[tq]} {'tr' if transpose else 'copy'} axis {axis}"
    got, exp, _, _ = _run_tiles(costa, tq, F, ops, m * n, m * n, m, n, 1.0, 0.0, axis, None, "line", FLOOR, False,
                                what, src=src, sa=sa)
    sub = exp[(exp != 0) & np.isfinite(exp) & (np.abs(exp) < 2.0 ** -126)]
    assert sub.size > 0 and np.isnan(exp).any() and np.isinf(exp).any()


# ------------------------------------------------------------------ transform_mx on one rank
def _scales_for(costa, case_shape, axis, order, init=None):
    rows, cols = case_shape
    shape = (mc.n_blocks(rows), cols) if axis == ROWS else (mc.n_blocks(cols), rows)
    return ScaleT(costa, axis, *shape, order, init=None if init is None else init(shape))


def _xf(costa, kind, tq, geom, op, a_axis=ROWS, c_axis=ROWS, rounding=FLOOR, alpha=1.0, beta=0.0, order="block",
        stream=None, comm=None):
    """one one-rank transform_mx against the model -> what it checked"""
    ta, tc = {"quantise": (F, tq), "dequantise": (tq, F), "requantise": (tq, tq)}[kind]
    a_case, c_case = mc.geometry(geom, op)
    what = f"{kind} {NAMES[ta]}->{NAMES[tc]} {geom} {op}"
    na, nc = a_case.buf_elems(0, 1), c_case.buf_elems(0, 1)
    a = mc.quant_data(0x31, na) if ta == F else _fp8_data(ta, 0x32, na)
    c = mc.fc.gen(tc, 0x33, nc)
    SA = _scales_for(costa, a_case.shape(), a_axis, order, lambda s: mc.scale_bytes(0x34, s)) if ta != F else None
    SC = _scales_for(costa, c_case.shape(), c_axis, order) if tc != F else None
    exp, esc, t = mc.expected_transform_mx(ta, tc, op, alpha, beta, a_case, c_case, 1, [a], [c],
                                           sa=SA.init if SA else None, a_axis=a_axis,
                                           c_axis=c_axis if SC else None, rounding=rounding)
    da, dc = dev(a), dev(c)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    comm = comm or costa.Comm.self(0)
    costa.transform_mx(A, C, comm, op, alpha, beta, a_scales=SA.desc if SA else None,
                       c_scales=SC.desc if SC else None, rounding=RND[rounding], stream=stream)
    if stream is not None:
        stream.synchronize()
    if SC:
        SC.check(esc, what + ": c_scales")
        mc.assert_data_finite(exp[0], tc, what)
    if SA:
        SA.check(SA.init, what + ": a_scales")
    assert_bits(host(dc, tc), exp[0], tc, what)
    assert da.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    return t


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["g192", "g203", "g203pad", "custom32"])
@pytest.mark.parametrize("kind", ["quantise", "dequantise", "requantise"])
def test_transform_mx_one_rank(costa, kind, geom, op):
    tq = E4M3 if geom in ("g192", "g203pad") else E5M2
    rounding = CEIL if geom == "g203pad" else FLOOR
    # requantise 'T' turns the block axis round ('N' keeps it); the others alternate with the geometry
    a_axis = ROWS if geom in ("g192", "custom32") else COLS
    c_axis = (COLS if a_axis == ROWS else ROWS) if kind == "requantise" and op == "T" else a_axis
    alpha, beta = (-0.5, 2.0) if kind == "dequantise" and op == "T" else (1.0, 0.0) if op == "N" else (0.75, 0.0)
    t = _xf(costa, kind, tq, geom, op, a_axis, c_axis, rounding, alpha, beta, order="block" if op == "N" else "line")
    if kind == "quantise" and rounding == FLOOR:  # (fp32 data: some elements saturate; FP8 sources times a
        assert (np.abs(t) > float(mc.FMAX[tq])).any()  # power of two need not, the tile lists cover those)


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["bc203", "cfg5"])
def test_dequantise_any_layout_pair(costa, geom, op):
    """a_scales has no tile-boundary restriction: unaligned blocks index per element"""
    _xf(costa, "dequantise", E4M3, geom, op, a_axis=ROWS if op == "N" else COLS, alpha=-0.5, beta=2.0)


@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
def test_requantise_transposed_keeps_cols_blocks(costa, tq):
    """'T' from axis COLS of A to axis COLS of the transposed matrix: not a byte transpose, the model's
    dequantise-then-quantise"""
    _xf(costa, "requantise", tq, "g203", "T", a_axis=COLS, c_axis=COLS)


def test_transform_mx_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _xf(costa, "quantise", E4M3, "g203", "T", c_axis=COLS, alpha=0.75, stream=s)
        _xf(costa, "dequantise", E5M2, "g192", "N", a_axis=ROWS, alpha=-0.5, beta=2.0, stream=s)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_unchanged(costa):
    comm = costa.Comm.self(0)
    a_case, c_case = mc.geometry("g192", "N")
    m, n = c_case.shape()
    nel = {F: mc.quant_data(1, a_case.buf_elems(0, 1)), E4M3: _fp8_data(E4M3, 2, a_case.buf_elems(0, 1)),
           E5M2: _fp8_data(E5M2, 3, a_case.buf_elems(0, 1))}
    sc0 = np.full((mc.n_blocks(m), n), 0x5A, np.uint8)
    dsa, dsc = dev(sc0), dev(sc0)
    SA = costa.mx_scales(dsa.view(mc.n_blocks(m), n), "rows")
    SC = costa.mx_scales(dsc.view(mc.n_blocks(m), n), "rows")

    def lay(case, code, buf):
        return make_layout(costa, case, 0, buf.data_ptr(), 1, code)

    def refused(ta, tc, match, a_scales, c_scales, alpha=1.0, beta=0.0, cases=(a_case, c_case), names=True):
        c0 = np.resize(np.arange(251, dtype=np.uint8), cases[1].buf_elems(0, 1) * 8)
        da, dc = dev(np.resize(nel.get(ta, nel[F]).view(np.uint8), cases[0].buf_elems(0, 1) * 8)), dev(c0)
        with pytest.raises(costa.CostaError, match=match) as e:
            costa.transform_mx(lay(cases[0], ta, da), lay(cases[1], tc, dc), comm, "N", alpha, beta,
                               a_scales=a_scales, c_scales=c_scales)
        assert e.value.code == 1, str(e.value)
        if names:
            assert mc.fc.CNAMES[ta] in str(e.value) and mc.fc.CNAMES[tc] in str(e.value), str(e.value)
        assert dc.cpu().numpy().tobytes() == c0.tobytes()
        assert dsa.cpu().numpy().tobytes() == sc0.tobytes() and dsc.cpu().numpy().tobytes() == sc0.tobytes()

    # every unsupported pair, with both type names
    D, H, B = costa.DOUBLE, costa.HALF, costa.BFLOAT16
    for ta, tc in ((F, F), (D, D), (F, D), (D, E4M3), (E4M3, D), (H, E4M3), (E4M3, B), (B, B), (E4M3, E5M2),
                   (E5M2, E4M3), (costa.CFLOAT, costa.CFLOAT)):
        refused(ta, tc, "no MX transform", SA if ta in QS else None, SC if tc in QS else None)
    # beta != 0 with c_scales
    refused(F, E4M3, "beta must be 0", None, SC, beta=2.0, names=False)
    refused(E5M2, E5M2, "beta must be 0", SA, SC, beta=-1.0, names=False)
    # a missing or a superfluous descriptor
    refused(F, E4M3, "c_scales is required", None, None)
    refused(F, E4M3, "a_scales given", SA, SC)
    refused(E4M3, F, "a_scales is required", None, None)
    refused(E4M3, F, "c_scales given", SA, SC)
    refused(E5M2, E5M2, "a_scales is required", None, SC)
    refused(E5M2, E5M2, "c_scales is required", SA, None)
    # strides
    refused(F, E4M3, "strides", None, costa.MxScales(dsc.data_ptr(), ROWS, 1, 1), names=False)
    refused(F, E4M3, "strides", None, costa.MxScales(dsc.data_ptr(), ROWS, 0, 1), names=False)
    # C blocks of 40 x 24 split MX blocks, along either axis; dequantise of the same pair is fine
    bc = mc.geometry("bc203", "N")
    m2, n2 = bc[1].shape()
    big = dev(np.full(max(m2, n2) * 8, 0x5A, np.uint8))
    for axis, shape in ((ROWS, (mc.n_blocks(m2), n2)), (COLS, (mc.n_blocks(n2), m2))):
        d = costa.MxScales(big.data_ptr(), axis, shape[1], 1)
        refused(F, E4M3, "MX block", None, d, cases=bc, names=False)
        refused(E5M2, E5M2, "MX block", d, d, cases=bc, names=False)
    assert big.cpu().numpy().tobytes() == bytes([0x5A]) * (max(m2, n2) * 8)
    # a host pointer
    hs = sc0.copy()
    refused(F, E4M3, "device-resident", None, costa.MxScales(hs.ctypes.data, ROWS, n, 1), names=False)
    refused(E4M3, F, "device-resident", costa.MxScales(hs.ctypes.data, ROWS, n, 1), None, names=False)
    assert hs.tobytes() == sc0.tobytes()
    # host-resident layouts
    ha, hc = nel[F].copy(), np.zeros(c_case.buf_elems(0, 1), np.uint8)
    with pytest.raises(costa.CostaError, match="device-resident"):
        costa.transform_mx(make_layout(costa, a_case, 0, ha.ctypes.data, 1, F),
                           make_layout(costa, c_case, 0, hc.ctypes.data, 1, E4M3), comm, c_scales=SC)
    assert not hc.any() and dsc.cpu().numpy().tobytes() == sc0.tobytes()
    # the Python checks of mx_scales
    for bad in (torch.zeros(mc.n_blocks(m), n, dtype=torch.uint8), torch.zeros(mc.n_blocks(m), n, device="cuda"),
                torch.zeros(n, dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            costa.mx_scales(bad, "rows")
    with pytest.raises(ValueError):
        costa.mx_scales(dsc.view(mc.n_blocks(m), n), "rows", shape=(m + 40, n))
    with pytest.raises(ValueError):  # the extent is checked against C's matrix
        da, dc = dev(nel[F]), dev(np.zeros(c_case.buf_elems(0, 1), np.uint8))
        costa.transform_mx(lay(a_case, F, da), lay(c_case, E4M3, dc), comm, c_scales=costa.mx_scales(
            torch.zeros(mc.n_blocks(m) + 1, n, dtype=torch.uint8, device="cuda"), "rows"))
    # tile lists: a split block and beta != 0 are refused there too
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, 40, 8, 40, 40, ALPHA << 4 | F_ROWS, 0), 0, 0)
    dd = dev(np.zeros(4096, np.uint8))
    for o, match in ((ops, "MX block"),):
        with pytest.raises(costa.CostaError, match=match):
            costa.execute_tiles_mx(F, E4M3, o, [1, 0], 64, 8, dev(nel[F]).data_ptr(), dd.data_ptr(), c_scales=SC)
    ops["op"]["nf"], ops["op"]["flags"] = 32, AXPBY << 4 | F_ROWS
    with pytest.raises(costa.CostaError, match="beta must be 0"):
        costa.execute_tiles_mx(F, E4M3, ops, [1, 2], 64, 8, dev(nel[F]).data_ptr(), dd.data_ptr(), c_scales=SC)
    assert not dd.cpu().numpy().any() and dsc.cpu().numpy().tobytes() == sc0.tobytes()
    # and the calls work afterwards
    _xf(costa, "quantise", E4M3, "g192", "N", comm=comm)


# ------------------------------------------------------------------ several ranks on one GPU
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", ["quantise", "dequantise"])
def test_emulated_ranks_2x2(costa, kind, op):
    """quantise sends fp32 packages, dequantise Q packages (a_scales complete on every rank); each
    rank's c_scales holds exactly its own blocks' bytes over a zero fill and their maximum is the
    model's tensor"""
    tq, P = E4M3, 4
    ta, tc = (F, tq) if kind == "quantise" else (tq, F)
    a_case, c_case = mc.geometry("g203", op, (2, 2))
    m, n = c_case.shape()
    alpha, beta = (0.75, 0.0) if kind == "quantise" else (-0.5, 2.0)
    a = [mc.quant_data(0x40 + r, a_case.buf_elems(r, P)) if ta == F else _fp8_data(ta, 0x40 + r, a_case.buf_elems(r, P))
         for r in range(P)]
    c = [mc.fc.gen(tc, 0x50 + r, c_case.buf_elems(r, P)) for r in range(P)]
    axis = COLS if op == "T" else ROWS
    am, an = a_case.shape()
    sa_shape = (mc.n_blocks(am), an) if axis == ROWS else (mc.n_blocks(an), am)
    sc_shape = (mc.n_blocks(m), n) if axis == ROWS else (mc.n_blocks(n), m)
    sa = mc.scale_bytes(0x66, sa_shape) if ta != F else None
    exp, esc, _ = mc.expected_transform_mx(ta, tc, op, alpha, beta, a_case, c_case, P, a, c, sa=sa, a_axis=axis,
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

    out = drive(costa, plans, ESIZE[ta], call)
    assert out.stats["pack_launches"] > 0 and out.stats["unpack_launches"] > 0
    assert costa.mx_items() > i0 and costa.scaled_items() == s0
    for r in range(P):
        what = f"{kind} {op} rank {r}"
        if tc != F:
            mc.assert_data_finite(exp[r], tc, what)
        assert_bits(host(dc[r], tc), exp[r], tc, what)
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
def test_mx_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK on mx_kernel (tests/mx_loopback_child.py)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mx_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_ = out[-1].split()
    assert int(n) == 3 and int(packs) > 0 and int(unpacks) > 0, out[-1]
    assert (int(locals_) == 0) == (mode == "1"), out[-1]


# ------------------------------------------------------------------ neighbours
def test_other_transforms_are_unchanged_around_an_mx_call(costa):
    """ordinary, scaled and amax calls on the same layout handles give identical bytes before and after
    MX calls; the MX calls add no second plan for the pair and count their own sub-tiles"""
    a_case, c_case = mc.geometry("g203", "T")
    m, n = c_case.shape()
    comm = costa.Comm.self(0)
    a = mc.quant_data(0x61, a_case.buf_elems(0, 1))
    c0 = mc.fc.gen(E4M3, 0x62, c_case.buf_elems(0, 1))
    r = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 2, m).astype(np.float32)).cuda()
    da, dc = dev(a), dev(c0)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, F)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, E4M3)

    def others():
        out = []
        for which in ("plain", "scaled", "amax"):
            dc.copy_(dev(c0))
            ra = torch.zeros(m, dtype=torch.float32, device="cuda")
            if which == "plain":
                costa.transform(A, C, comm, "T", 0.75, 0.0)
            elif which == "scaled":
                costa.transform_scaled(A, C, comm, "T", 0.75, 0.0, row_scale=r)
            else:
                costa.transform_amax(A, C, comm, "T", 0.75, 0.0, row_scale=r, row_amax=ra)
            out.append(dc.cpu().numpy().tobytes() + ra.cpu().numpy().tobytes())
        return out
    before = others()
    st0 = costa.get_stats()
    SC = _scales_for(costa, (m, n), COLS, "block")
    i0, s0, a0 = costa.mx_items(), costa.scaled_items(), costa.amax_items()
    dc.copy_(dev(c0))
    costa.transform_mx(A, C, comm, "T", 0.75, 0.0, c_scales=SC.desc)
    exp, esc, _ = mc.expected_transform_mx(F, E4M3, "T", 0.75, 0.0, a_case, c_case, 1, [a], [c0], c_axis=COLS)
    SC.check(esc, "mx in between")
    assert_bits(host(dc, E4M3), exp[0], E4M3, "mx in between")
    assert costa.mx_items() - i0 > 0 and costa.scaled_items() == s0 and costa.amax_items() == a0
    SC2 = _scales_for(costa, (m, n), ROWS, "line")
    costa.transform_mx(A, C, comm, "T", 0.75, 0.0, c_scales=SC2.desc, rounding="ceil")
    st1 = costa.get_stats()
    # the scaled plan of the pair was already there: the MX calls are plan-cache hits
    assert st1["plan_misses"] == st0["plan_misses"] and st1["plan_hits"] - st0["plan_hits"] == 2
    s1 = costa.scaled_items()
    assert others() == before
    assert costa.scaled_items() > s1
    ref = mc.widen(c0, E4M3)
    oracle.transform(oracle.FLOAT, "T", 0.75, 0.0, a_case.geom(1), [a], c_case.geom(1), [ref])
    assert before[0][:c0.size] == mc.cvt(ref, E4M3).tobytes()
