"""Block-scaled FP8 transforms on the GPU (costa_hip.h, "Block-scaled FP8 transforms (fp32 scales)"):
block_kernel through costa_hip_execute_tiles_block_scaled, and costa_hip_transform_block_scaled on one
rank, on a stream, on emulated ranks and through the loopback exchange.  Expected data bits and scale
floats come from the model of bs_common.py; everything is compared bit for bit over whole buffers, the
floats around the scale tensors included."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bs_common as bc
import oracle
from bs_common import E4M3, E5M2, EXACT, F, NAMES, POW2, RND, SHAPE_IDS, SHAPES, assert_bits, make_layout
from emulated_ranks import drive

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR, F_ROWS = 0x1, 0x80
BITCOPY, ALPHA, AXPBY = 0, 2, 3
ESIZE = {F: 4, E4M3: 1, E5M2: 1}
NPT = {F: np.float32, E4M3: np.uint8, E5M2: np.uint8}
QS = [E4M3, E5M2]
M, N = bc.M, bc.N


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
    """a scale tensor [block row, block column] inside a larger device buffer of fill floats: "row"
    (block columns consecutive, a gap of 3 floats after each block row) or "col" (block rows
    consecutive, a gap of 2 after each block column), 8 sentinel floats on each side"""
    PAD = 8

    def __init__(self, costa, block, shape, order, init=None, fill=-7.0):
        nbr, nbc = shape
        self.block, self.shape = block, shape
        if order == "row":
            self.rs, self.cs = nbc + 3, 1
            size = nbr * self.rs
        else:
            self.rs, self.cs = 1, nbr + 2
            size = nbc * self.cs
        self.at = (self.PAD + np.arange(nbr)[:, None] * self.rs + np.arange(nbc)[None, :] * self.cs).astype(np.int64)
        full = np.full(size + 2 * self.PAD, fill, np.float32)
        self.init = np.full(shape, fill, np.float32) if init is None else np.asarray(init, np.float32)
        full[self.at] = self.init
        self.full0 = full
        self.t = torch.from_numpy(full.copy()).cuda()
        self.desc = costa.BlockScales(self.t.data_ptr() + 4 * self.PAD, block[0], block[1], self.rs, self.cs)

    def check(self, exp, what):
        """the tensor holds `exp` exactly and every other float of the buffer is unchanged"""
        want = self.full0.copy()
        want[self.at] = exp
        bc.assert_float_bits(self.t.cpu().numpy(), want, what + " (with the floats around the tensor)")


# ------------------------------------------------------------------ kernel level: tile lists
# target regions (row0, col0, rows, cols, F_ROWS, source shift, destination shift) of the 330 x 270
# matrix that obey the rule of every block shape ...
COMMON = [
    (0, 0, 128, 128, True, 0, 0),        # one whole region (FULL path)
    (0, 128, 256, 128, False, 0, 0),     # 256 x 128: two whole regions along s
    (128, 0, 128, 128, False, 0, 3),     # destination off the 16-byte grid (guarded path)
    (256, 256, 74, 14, True, 0, 0),      # the corner: partial blocks along both dimensions
    (0, 256, 128, 14, False, 1, 0),      # the right edge, source off the grid
]
# ... and those of one shape only: 128 x 1 and 1 x 128 ops, and the bottom edge
EXTRA = {
    (128, 1): [(128, 256, 128, 1, True, 0, 0), (128, 257, 128, 13, False, 0, 0), (256, 3, 74, 250, True, 0, 0)],
    (1, 128): [(256, 0, 1, 128, False, 0, 0), (257, 0, 73, 256, True, 0, 0), (128, 256, 77, 14, True, 0, 0)],
    (128, 128): [(256, 0, 74, 256, True, 0, 0), (128, 256, 128, 14, True, 0, 0)],
}


def _tile_list(costa, block, transpose, kind, flip=False):
    """-> (ops with ELEMENT offsets, source elements, destination elements)"""
    regions = COMMON + EXTRA[block]
    ops = np.zeros(len(regions), costa.SCALED_OP_DTYPE)
    src_at = dst_at = 0
    for k, (r0, c0, nr, nc, frow, s_off, d_off) in enumerate(regions):
        frow = frow != flip
        nf, ns = (nr, nc) if frow else (nc, nr)

        def place(at, fast, slow, off):
            ld = (fast + 15) // 16 * 16 + (1 if off else 0)
            return at + off, ld, (at + off + ld * slow + 15) // 16 * 16
        s0, lds, src_at = place(src_at, nf, ns, s_off)
        df, dslow = (ns, nf) if transpose else (nf, ns)
        d0, ldd, dst_at = place(dst_at, df, dslow, d_off)
        flags = (TR if transpose else 0) | kind << 4 | (F_ROWS if frow else 0)
        ops[k] = ((s0, d0, nf, ns, lds, ldd, flags, 0), r0, c0)
    return ops, src_at + 16, dst_at + 16


def _items(ops, edge):
    return sum(-(-int(o["op"]["nf"]) // edge) * -(-int(o["op"]["ns"]) // edge) for o in ops)


def _gpu_ops(ops, ta, tc):
    g = ops.copy()
    g["op"]["src"] = ops["op"]["src"] * ESIZE[ta]
    g["op"]["dst"] = ops["op"]["dst"] * ESIZE[tc]
    return g


def _fp8_data(tq, seed, n):
    return bc.cvt(bc.quant_data(seed, n), tq)


def _run_tiles(costa, ta, tc, ops, n_src, n_dst, m, n, alpha, beta, a_block, c_block, order, rounding, a_tr, what,
               src=None, sa=None):
    scal = np.array([alpha, beta], np.float32)
    if src is None:
        src = bc.quant_data(0xA1, n_src) if ta == F else _fp8_data(ta, 0xA2, n_src)
    dst0 = bc.fc.gen(tc, 0xC1, n_dst)
    SA = SC = None
    if ta != F:
        shape = bc.n_blocks((n, m) if a_tr else (m, n), a_block)
        SA = ScaleT(costa, a_block, shape, order, init=bc.scale_floats(0x5A, shape) if sa is None else sa)
    if tc != F:
        SC = ScaleT(costa, c_block, bc.n_blocks((m, n), c_block), order)
    exp, esc, t = bc.expected_tiles_bs(ta, tc, ops, alpha, beta, src, dst0, m, n, sa=SA.init if SA else None,
                                       a_block=a_block, a_transposed=a_tr, c_block=c_block if SC else None,
                                       rounding=rounding, sc_fill=SC.init if SC else None)
    ds, dd = dev(src), dev(dst0)
    i0, s0, m0 = costa.block_items(), costa.scaled_items(), costa.mx_items()
    costa.execute_tiles_block_scaled(ta, tc, _gpu_ops(ops, ta, tc), scal, m, n, ds.data_ptr(), dd.data_ptr(),
                                     a_scales=SA.desc if SA else None, c_scales=SC.desc if SC else None,
                                     rounding=RND[rounding], a_transposed=a_tr)
    got = host(dd, tc)
    if SC:
        SC.check(esc, what + ": c_scales")
    if SA:
        SA.check(SA.init, what + ": a_scales")
    assert_bits(got, exp, tc, what + ": destination")
    assert costa.block_items() - i0 == _items(ops, 128 if SC else 64)
    assert costa.scaled_items() == s0 and costa.mx_items() == m0
    assert ds.cpu().numpy().tobytes() == np.ascontiguousarray(src).tobytes()
    return got, exp, esc, t


def _check_range(tc, got, exp, t, rounding, what):
    fm = float(bc.FMAX[tc])
    assert np.isfinite(bc.widen(exp, tc)).all(), what
    assert (np.abs(bc.widen(got, tc)) <= fm).all(), what
    if rounding == POW2:
        assert (np.abs(t) <= fm).all(), what


@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("rounding", [EXACT, POW2], ids=["exact", "pow2"])
@pytest.mark.parametrize("block", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("flip", [False, True], ids=["frows", "fcols"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_quantise_tile_lists(costa, transpose, flip, block, rounding, tq):
    what = f"quantise f32->{NAMES[tq]} {'tr' if transpose else 'copy'} flip {flip} {block} {RND[rounding]}"
    kind, alpha = (ALPHA, -0.5) if transpose else (BITCOPY, 1.0)
    ops, ns, nd = _tile_list(costa, block, transpose, kind, flip)
    order = "row" if (rounding == EXACT) != flip else "col"
    got, exp, esc, t = _run_tiles(costa, F, tq, ops, ns, nd, M, N, alpha, 0.0, None, block, order, rounding, False, what)
    _check_range(tq, got, exp, t, rounding, what)


@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("order", ["row", "col"])
@pytest.mark.parametrize("block", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("a_tr", [False, True], ids=["a", "at"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_dequantise_tile_lists(costa, transpose, a_tr, block, order, tq):
    """beta != 0: the old destination values are read; a_scales indexed by A's matrix, also turned round"""
    what = f"dequantise {NAMES[tq]}->f32 {'tr' if transpose else 'copy'} a_tr {a_tr} {block} {order}"
    ops, ns, nd = _tile_list(costa, (128, 128), transpose, AXPBY, flip=(order == "col"))
    got, exp, _, _ = _run_tiles(costa, tq, F, ops, ns, nd, M, N, -0.5, 2.0, block, None, order, EXACT, a_tr, what)
    assert np.isfinite(exp).all()


@pytest.mark.parametrize("c_block", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("a_block", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_requantise_tile_lists(costa, transpose, a_block, c_block):
    k = SHAPES.index(a_block) + SHAPES.index(c_block)
    tq, rounding = QS[k % 2], (EXACT, POW2)[(k // 2 + transpose) % 2]
    what = f"requantise {NAMES[tq]} {'tr' if transpose else 'copy'} {a_block}->{c_block} {RND[rounding]}"
    ops, ns, nd = _tile_list(costa, c_block, transpose, ALPHA, flip=bool(k % 2))
    got, exp, esc, t = _run_tiles(costa, tq, tq, ops, ns, nd, M, N, 0.75, 0.0, a_block, c_block,
                                  "row" if transpose else "col", rounding, transpose, what)
    _check_range(tq, got, exp, t, rounding, what)


# ------------------------------------------------------------------ specials, the division
@pytest.mark.parametrize("rounding", [EXACT, POW2], ids=["exact", "pow2"])
@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
@pytest.mark.parametrize("frow", [True, False], ids=["along-f", "along-s"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
def test_special_blocks(costa, transpose, frow, tq, rounding):
    """all-zero, below 2^-40, subnormal, NaN, inf, -0, the largest and the smallest normal amax: one
    128 x 1 block per column of 128 x 8, in a 128 x 10 matrix whose last two scales keep their fill"""
    V = bc.special_matrix()
    m, n = V.shape
    src = (V.T if frow else V).reshape(-1).copy()  # element (f, s) at s * lds + f
    nf, ns = (m, n) if frow else (n, m)
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, nf, ns, nf, ns if transpose else nf, (TR if transpose else 0) | BITCOPY << 4 |
               (F_ROWS if frow else 0), 0), 0, 0)
    what = f"specials {NAMES[tq]} {'tr' if transpose else 'copy'} frow {frow} {RND[rounding]}"
    got, exp, esc, t = _run_tiles(costa, F, tq, ops, src.size, m * n, m, n + 2, 1.0, 0.0, None, (128, 1), "row",
                                  rounding, False, what, src=src)
    S = esc[0].view(np.uint32)
    eps_s = (np.float32(2.0 ** -40) / bc.FMAX[tq]) if rounding == EXACT else np.float32(2.0 ** (-40 - bc.EMAX[tq]))
    assert (S[[0, 1, 2, 5]] == eps_s.view(np.uint32)).all()
    assert S[3] == 0x7FC00000 and S[4] == 0x7FC00000
    assert (S[8:] == np.float32(-7.0).view(np.uint32)).all()            # untouched: the fill
    assert np.isfinite(esc[0][[6, 7]]).all() and (esc[0][[6, 7]] >= np.float32(2.0 ** -126)).all()
    assert np.isnan(bc.widen(got, tq)).sum() == 2 * 128                  # the NaN and the inf block, nothing else


@pytest.mark.parametrize("tq", QS, ids=lambda c: NAMES[c])
def test_division_is_numpys_for_many_amax(costa, tq):
    """EXACT: S = amax_c / fmax and R = fmax / amax_c are numpy's fp32 quotients for 4096 amax values over
    every binade from below 2^-40 to the largest finite one (R shows in the data bits of the two
    elements beside the maximum)"""
    n = 4096
    rng = np.random.default_rng(0xD1)
    bits = (rng.integers(80, 255, n).astype(np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n).astype(np.uint32)
    amax = bits.view(np.float32)
    V = np.zeros((128, n), np.float32)
    rows = np.arange(n) % 126
    V[rows, np.arange(n)] = amax
    V[rows + 1, np.arange(n)] = -amax * np.float32(0.6180339)
    V[rows + 2, np.arange(n)] = amax * np.float32(0.0437)
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, 128, n, 128, 128, BITCOPY << 4 | F_ROWS, 0), 0, 0)
    src = V.T.reshape(-1).copy()
    got, exp, esc, t = _run_tiles(costa, F, tq, ops, src.size, 128 * n, 128, n, 1.0, 0.0, None, (128, 1), "row",
                                  EXACT, False, f"division {NAMES[tq]}", src=src)
    with np.errstate(all="ignore"):
        want = np.maximum(amax, np.float32(2.0 ** -40)) / bc.FMAX[tq]
    assert (esc[0].view(np.uint32) == want.view(np.uint32)).all()


# ------------------------------------------------------------------ transform_block_scaled on one rank
def _scales_for(costa, case_shape, block, order, init=None, fill=-7.0):
    shape = bc.n_blocks(case_shape, block)
    return ScaleT(costa, block, shape, order, init=None if init is None else init(shape), fill=fill)


def _xf(costa, kind, tq, geom, op, a_block=(1, 128), c_block=(1, 128), rounding=EXACT, alpha=1.0, beta=0.0,
        order="row", stream=None, comm=None):
    """one one-rank transform_block_scaled against the model"""
    ta, tc = {"quantise": (F, tq), "dequantise": (tq, F), "requantise": (tq, tq)}[kind]
    a_case, c_case = bc.geometry(geom, op)
    what = f"{kind} {NAMES[ta]}->{NAMES[tc]} {geom} {op} {a_block}->{c_block}"
    na, nc = a_case.buf_elems(0, 1), c_case.buf_elems(0, 1)
    a = bc.quant_data(0x31, na) if ta == F else _fp8_data(ta, 0x32, na)
    c = bc.fc.gen(tc, 0x33, nc)
    SA = _scales_for(costa, a_case.shape(), a_block, order, lambda s: bc.scale_floats(0x34, s)) if ta != F else None
    SC = _scales_for(costa, c_case.shape(), c_block, order) if tc != F else None
    exp, esc, t = bc.expected_transform_bs(ta, tc, op, alpha, beta, a_case, c_case, 1, [a], [c],
                                           sa=SA.init if SA else None, a_block=a_block,
                                           c_block=c_block if SC else None, rounding=rounding)
    da, dc = dev(a), dev(c)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    comm = comm or costa.Comm.self(0)
    costa.transform_block_scaled(A, C, comm, op, alpha, beta, a_scales=SA.desc if SA else None,
                                 c_scales=SC.desc if SC else None, rounding=RND[rounding], stream=stream)
    if stream is not None:
        stream.synchronize()
    if SC:
        SC.check(esc, what + ": c_scales")
        assert np.isfinite(bc.widen(exp[0], tc)).all()
    if SA:
        SA.check(SA.init, what + ": a_scales")
    assert_bits(host(dc, tc), exp[0], tc, what)
    assert da.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["bc128", "bc128pad", "custom128"])
@pytest.mark.parametrize("kind", ["quantise", "dequantise", "requantise"])
def test_transform_one_rank(costa, kind, geom, op):
    g = ["bc128", "bc128pad", "custom128"].index(geom)
    tq = QS[g % 2]
    rounding = POW2 if geom == "bc128pad" else EXACT
    a_block = SHAPES[g]
    # requantise 'T' cuts 1 x 128 groups of A anew along the other dimension of the transposed matrix
    c_block = (1, 128) if kind == "requantise" and op == "T" and a_block == (1, 128) else SHAPES[(g + (op == "T")) % 3]
    alpha, beta = (-0.5, 2.0) if kind == "dequantise" and op == "T" else (1.0, 0.0) if op == "N" else (0.75, 0.0)
    _xf(costa, kind, tq, geom, op, a_block, c_block, rounding, alpha, beta, order="row" if op == "N" else "col")


@pytest.mark.parametrize("block", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("op", ["N", "T"])
def test_dequantise_any_layout_pair(costa, op, block):
    """a_scales has no tile-boundary restriction: blocks of 40 x 24 index per element"""
    _xf(costa, "dequantise", E4M3, "bc203", op, a_block=block, alpha=-0.5, beta=2.0)


def test_transform_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _xf(costa, "quantise", E4M3, "bc128", "T", c_block=(128, 128), alpha=0.75, stream=s)
        _xf(costa, "dequantise", E5M2, "custom128", "N", a_block=(128, 1), alpha=-0.5, beta=2.0, stream=s)


# ------------------------------------------------------------------ refusals
CN = dict(bc.fc.CNAMES)
CN.update({9: "FP4_E2M1", 10: "FP6_E2M3", 11: "FP6_E3M2"})


def test_refusals_leave_everything_unchanged(costa):
    comm = costa.Comm.self(0)
    a_case, c_case = bc.geometry("bc128", "N")
    m, n = c_case.shape()
    na = a_case.buf_elems(0, 1)
    nel = {F: bc.quant_data(1, na), E4M3: _fp8_data(E4M3, 2, na), E5M2: _fp8_data(E5M2, 3, na)}
    sc0 = np.full(bc.n_blocks((m, n), (1, 128)), 0.375, np.float32)
    dsa, dsc = torch.from_numpy(sc0.copy()).cuda(), torch.from_numpy(sc0.copy()).cuda()
    SA = costa.block_scales(dsa, (1, 128))
    SC = costa.block_scales(dsc, (1, 128))

    def lay(case, code, buf):
        return make_layout(costa, case, 0, buf.data_ptr(), 1, code)

    def refused(ta, tc, match, a_scales, c_scales, alpha=1.0, beta=0.0, cases=(a_case, c_case), names=True,
                rounding="exact", same=False, uplo=None):
        c0 = np.resize(np.arange(251, dtype=np.uint8), cases[1].buf_elems(0, 1) * 8)
        da, dc = dev(np.resize(nel.get(ta, nel[F]).view(np.uint8), cases[0].buf_elems(0, 1) * 8)), dev(c0)
        A, C = lay(cases[0], ta, da), lay(cases[1], tc, dc)
        with pytest.raises(costa.CostaError, match=match) as e:
            costa.transform_block_scaled(A, A if same else C, comm, "N", alpha, beta, a_scales=a_scales,
                                         c_scales=c_scales, rounding=rounding)
        assert e.value.code == 1, str(e.value)
        if names:
            assert CN[ta] in str(e.value) and CN[tc] in str(e.value), str(e.value)
        assert dc.cpu().numpy().tobytes() == c0.tobytes()
        assert dsa.cpu().numpy().tobytes() == sc0.tobytes() and dsc.cpu().numpy().tobytes() == sc0.tobytes()

    # every unsupported pair, with both type names
    D, H, B, I = costa.DOUBLE, costa.HALF, costa.BFLOAT16, costa.INT32
    for ta, tc in ((F, F), (D, D), (F, D), (D, E4M3), (E4M3, D), (H, E4M3), (E4M3, B), (B, B), (E4M3, E5M2),
                   (E5M2, E4M3), (costa.CFLOAT, costa.CFLOAT), (costa.CDOUBLE, E4M3), (I, I), (I, E5M2)):
        refused(ta, tc, "no block-scaled transform", SA if ta in QS else None, SC if tc in QS else None)
    # the packed types, on a geometry their layouts accept (every extent a multiple of 4)
    from casegen import BC
    pk = (BC(256, 128, 128, 128), BC(256, 128, 128, 128))
    for ta, tc in ((F, costa.FP4_E2M1), (costa.FP4_E2M1, F), (costa.FP6_E2M3, costa.FP6_E2M3), (F, costa.FP6_E3M2),
                   (costa.FP4_E2M1, E4M3)):
        refused(ta, tc, "no block-scaled transform", None, None, cases=pk)
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
    # an unknown rounding value, an in-place call
    refused(F, E4M3, "rounding must be", None, SC, rounding=2, names=False)
    refused(E4M3, E4M3, "in-place", SA, SC, same=True, names=False)
    # block shape, strides, alignment
    refused(F, E4M3, "block shape", None, costa.BlockScales(dsc.data_ptr(), 128, 64, 3, 1), names=False)
    refused(F, E4M3, "block shape", None, costa.BlockScales(dsc.data_ptr(), 32, 1, 3, 1), names=False)
    refused(F, E4M3, "strides", None, costa.BlockScales(dsc.data_ptr(), 1, 128, 1, 1), names=False)
    refused(F, E4M3, "strides", None, costa.BlockScales(dsc.data_ptr(), 1, 128, 0, 1), names=False)
    refused(E4M3, F, "strides", costa.BlockScales(dsa.data_ptr(), 128, 128, 3, -1), None, names=False)
    refused(F, E4M3, "4-byte aligned", None, costa.BlockScales(dsc.data_ptr() + 2, 1, 128, 3, 1), names=False)
    # C blocks of 40 x 24 split scale blocks, for every shape; dequantise of the same pair is fine
    off = bc.geometry("bc203", "N")
    m2, n2 = off[1].shape()
    big = torch.full((max(m2, n2) * 4,), 0.375, dtype=torch.float32, device="cuda")
    for block in SHAPES:
        nbr, nbc = bc.n_blocks((m2, n2), block)
        d = costa.BlockScales(big.data_ptr(), block[0], block[1], nbc, 1)
        refused(F, E4M3, r"scale block.*(rows|columns) \d+ \.\. \d+ of \d+", None, d, cases=off, names=False)
        refused(E5M2, E5M2, "scale block", d, d, cases=off, names=False)
    assert (big.cpu().numpy() == np.float32(0.375)).all()
    # a host pointer
    hs = sc0.copy()
    refused(F, E4M3, "device-resident", None, costa.BlockScales(hs.ctypes.data, 1, 128, 3, 1), names=False)
    refused(E4M3, F, "device-resident", costa.BlockScales(hs.ctypes.data, 1, 128, 3, 1), None, names=False)
    assert hs.tobytes() == sc0.tobytes()
    # host-resident layouts
    ha, hc = nel[F].copy(), np.zeros(c_case.buf_elems(0, 1), np.uint8)
    with pytest.raises(costa.CostaError, match="device-resident"):
        costa.transform_block_scaled(make_layout(costa, a_case, 0, ha.ctypes.data, 1, F),
                                     make_layout(costa, c_case, 0, hc.ctypes.data, 1, E4M3), comm, c_scales=SC)
    assert not hc.any() and dsc.cpu().numpy().tobytes() == sc0.tobytes()
    # a batch
    with pytest.raises(costa.CostaError, match="batches"):
        costa.transform_block_scaled([None], [None], comm, c_scales=SC)
    # the Python checks of block_scales
    for bad in (torch.zeros(m, 3), torch.zeros(m, 3, dtype=torch.float16, device="cuda"),
                torch.zeros(m, device="cuda")):
        with pytest.raises(ValueError):
            costa.block_scales(bad, (1, 128))
    with pytest.raises(ValueError):
        costa.block_scales(dsc, (1, 64))
    with pytest.raises(ValueError):
        costa.block_scales(dsc, (1, 128), shape=(m + 40, n))
    with pytest.raises(ValueError):  # the extent is checked against C's matrix
        da, dc = dev(nel[F]), dev(np.zeros(c_case.buf_elems(0, 1), np.uint8))
        costa.transform_block_scaled(lay(a_case, F, da), lay(c_case, E4M3, dc), comm, c_scales=costa.block_scales(
            torch.zeros(m + 1, 3, device="cuda"), (1, 128)))
    # tile lists: a split block and beta != 0 are refused there too
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, 128, 64, 128, 128, ALPHA << 4 | F_ROWS, 0), 0, 0)
    dd = dev(np.zeros(1 << 15, np.uint8))
    with pytest.raises(costa.CostaError, match="scale block"):
        costa.execute_tiles_block_scaled(F, E4M3, ops, [1, 0], m, n, dev(nel[F]).data_ptr(), dd.data_ptr(), c_scales=SC)
    with pytest.raises(ValueError):  # (a rounding of the MX calls)
        costa.execute_tiles_block_scaled(F, E4M3, ops, [1, 0], m, n, 0, dd.data_ptr(), c_scales=SC, rounding="floor")
    ops["op"]["ns"], ops["op"]["flags"] = 128, AXPBY << 4 | F_ROWS
    with pytest.raises(costa.CostaError, match="beta must be 0"):
        costa.execute_tiles_block_scaled(F, E4M3, ops, [1, 2], m, n, dev(nel[F]).data_ptr(), dd.data_ptr(), c_scales=SC)
    with pytest.raises(costa.CostaError, match="no block-scaled kernel"):
        costa.execute_tiles_block_scaled(E4M3, E5M2, ops, [1, 0], m, n, dev(nel[F]).data_ptr(), dd.data_ptr(),
                                         a_scales=SA, c_scales=SC)
    assert not dd.cpu().numpy().any() and dsc.cpu().numpy().tobytes() == sc0.tobytes()
    # and the calls work afterwards
    _xf(costa, "quantise", E4M3, "bc128", "N", comm=comm)


# ------------------------------------------------------------------ several ranks on one GPU
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", ["quantise", "dequantise"])
def test_emulated_ranks_2x2(costa, kind, op):
    """quantise sends fp32 packages, dequantise Q packages (a_scales complete on every rank); each
    rank's c_scales holds exactly its own blocks' scales over a zero fill and their maximum is the
    model's tensor"""
    tq, P = E4M3, 4
    ta, tc = (F, tq) if kind == "quantise" else (tq, F)
    a_case, c_case = bc.geometry("bc128", op, (2, 2))
    m, n = c_case.shape()
    alpha, beta = (0.75, 0.0) if kind == "quantise" else (-0.5, 2.0)
    a = [bc.quant_data(0x40 + r, a_case.buf_elems(r, P)) if ta == F else _fp8_data(ta, 0x40 + r, a_case.buf_elems(r, P))
         for r in range(P)]
    c = [bc.fc.gen(tc, 0x50 + r, c_case.buf_elems(r, P)) for r in range(P)]
    block = (128, 128) if op == "T" else (1, 128)
    sa_shape, sc_shape = bc.n_blocks(a_case.shape(), block), bc.n_blocks((m, n), block)
    sa = bc.scale_floats(0x66, sa_shape) if ta != F else None
    exp, esc, _ = bc.expected_transform_bs(ta, tc, op, alpha, beta, a_case, c_case, P, a, c, sa=sa, a_block=block,
                                           c_block=block if tc != F else None)
    da, dc = [dev(x) for x in a], [dev(x) for x in c]
    lay = [(make_layout(costa, a_case, r, da[r].data_ptr(), P, ta), make_layout(costa, c_case, r, dc[r].data_ptr(), P, tc))
           for r in range(P)]
    plans = [costa.plan_export_scaled(lay[r][0], lay[r][1], r, P, op, alpha, beta) for r in range(P)]
    assert all(p.send_elems > 0 and p.recv_elems > 0 for p in plans)
    SA = [ScaleT(costa, block, sa_shape, "col", init=sa) if ta != F else None for r in range(P)]
    SC = [ScaleT(costa, block, sc_shape, "row", fill=0.0) if tc != F else None for r in range(P)]
    i0, s0, m0 = costa.block_items(), costa.scaled_items(), costa.mx_items()

    def call(r, comm):
        costa.transform_block_scaled(lay[r][0], lay[r][1], comm, op, alpha, beta,
                                     a_scales=SA[r].desc if SA[r] else None, c_scales=SC[r].desc if SC[r] else None)

    out = drive(costa, plans, ESIZE[ta], call)
    assert out.stats["pack_launches"] > 0 and out.stats["unpack_launches"] > 0
    assert costa.block_items() > i0 and costa.scaled_items() == s0 and costa.mx_items() == m0
    for r in range(P):
        what = f"{kind} {op} rank {r}"
        assert_bits(host(dc[r], tc), exp[r], tc, what)
    if tc != F:
        assert np.isfinite(esc).all() and (esc > 0).all()
        merged = np.zeros(sc_shape, np.float32)
        n_own = 0
        for r in range(P):
            first = bc.owned(c_case, P, r)[::block[0], ::block[1]]   # the rank owns a block with its first element
            mine = np.where(first, esc, np.float32(0)).astype(np.float32)
            SC[r].check(mine, f"{kind} {op} rank {r}: c_scales")
            merged = np.maximum(merged, mine)
            n_own += int(first.sum())
        assert n_own == esc.size and merged.tobytes() == esc.tobytes()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK on block_kernel (tests/bs_loopback_child.py)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bs_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_ = out[-1].split()
    assert int(n) == 3 and int(packs) > 0 and int(unpacks) > 0, out[-1]
    assert (int(locals_) == 0) == (mode == "1"), out[-1]


# ------------------------------------------------------------------ neighbours
def test_other_transforms_are_unchanged_around_a_block_scaled_call(costa):
    """ordinary, scaled and MX calls on the same layout handles give identical bytes before and after
    block-scaled calls; those add no second plan for the pair and count their own work items"""
    a_case, c_case = bc.geometry("bc128", "T")
    m, n = c_case.shape()
    comm = costa.Comm.self(0)
    a = bc.quant_data(0x61, a_case.buf_elems(0, 1))
    c0 = bc.fc.gen(E4M3, 0x62, c_case.buf_elems(0, 1))
    r = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 2, m).astype(np.float32)).cuda()
    da, dc = dev(a), dev(c0)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, F)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, E4M3)

    def others():
        out = []
        for which in ("plain", "scaled", "mx"):
            dc.copy_(dev(c0))
            e8 = torch.zeros((m + 31) // 32, n, dtype=torch.uint8, device="cuda")
            if which == "plain":
                costa.transform(A, C, comm, "T", 0.75, 0.0)
            elif which == "scaled":
                costa.transform_scaled(A, C, comm, "T", 0.75, 0.0, row_scale=r)
            else:
                costa.transform_mx(A, C, comm, "T", 0.75, 0.0, c_scales=costa.mx_scales(e8, "rows", (m, n)))
            out.append(dc.cpu().numpy().tobytes() + e8.cpu().numpy().tobytes())
        return out
    before = others()
    st0 = costa.get_stats()
    i0, s0, m0 = costa.block_items(), costa.scaled_items(), costa.mx_items()
    for block, rnd in (((128, 128), EXACT), ((1, 128), POW2), ((128, 1), EXACT)):
        SC = _scales_for(costa, (m, n), block, "row")
        dc.copy_(dev(c0))
        costa.transform_block_scaled(A, C, comm, "T", 0.75, 0.0, c_scales=SC.desc, rounding=RND[rnd])
        exp, esc, _ = bc.expected_transform_bs(F, E4M3, "T", 0.75, 0.0, a_case, c_case, 1, [a], [c0], c_block=block,
                                               rounding=rnd)
        SC.check(esc, f"block-scaled in between {block}")
        assert_bits(host(dc, E4M3), exp[0], E4M3, f"block-scaled in between {block}")
    assert costa.block_items() - i0 > 0 and costa.scaled_items() == s0 and costa.mx_items() == m0
    st1 = costa.get_stats()
    # the scaled plan of the pair was already there: the block-scaled calls are plan-cache hits
    assert st1["plan_misses"] == st0["plan_misses"] and st1["plan_hits"] - st0["plan_hits"] == 3
    assert others() == before
    ref = bc.widen(c0, E4M3)
    oracle.transform(oracle.FLOAT, "T", 0.75, 0.0, a_case.geom(1), [a], c_case.geom(1), [ref])
    assert before[0][:c0.size] == bc.cvt(ref, E4M3).tobytes()
