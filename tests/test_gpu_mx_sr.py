"""Stochastic rounding in the MX transforms on the GPU (costa_hip.h, "Stochastic rounding in the MX
transforms"): the SR instances of mx_kernel through costa_hip_execute_tiles_mx_sr, and
costa_hip_transform_mx_sr on one rank, on a stream, on emulated ranks and through the loopback exchange.
Expected codes come from the table model of mx_sr_common.py at the GLOBAL coordinates of C's matrix;
every comparison is bit for bit over the whole destination buffer, and scale bytes are compared
exactly, with the model's and with the bytes the call without a seed writes.

Every data comparison but the special blocks first asserts on the model that it cannot hide a failure
(`_model_ok`): the expected buffer is finite; of the elements whose t is not representable at least
20 % round down and at least 20 % up; the SR codes differ from the round-to-nearest codes in at least
10 % of the elements, so a kernel that ignores the seed fails."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fp4_common as f4
import fp6_common as f6
import mx_common as mc
import mx_sr_common as sr
from emulated_ranks import drive
from mx_sr_common import CEIL, COLS, E2M3, E3M2, E4M3, E5M2, F, FLOOR, FP4, NAMES, QTYPES, ROWS
from test_gpu_mx import ScaleT, dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR, F_ROWS = 0x1, 0x80
BITCOPY, ALPHA, AXPBY = 0, 2, 3
RND = {FLOOR: "floor", CEIL: "ceil"}
TYPES = pytest.mark.parametrize("tq", QTYPES, ids=[NAMES[t] for t in QTYPES])
# the matrix of the tile lists per type: 203 x 157 (FP8), 202 x 158 (FP4: even), 204 x 156 (FP6: multiples of 4)
DIMS = {E4M3: (203, 157), E5M2: (203, 157), FP4: (202, 158), E2M3: (204, 156), E3M2: (204, 156)}
GROUP = {E4M3: 1, E5M2: 1, FP4: 2, E2M3: 4, E3M2: 4}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def host(t):
    return t.cpu().numpy().view(np.uint8)


def _model_ok(r, tc, what):
    for e in (r.exp if isinstance(r.exp, list) else [r.exp]):
        sr.assert_finite(e, tc, what)
    r.shares.check(what)


def _seed(*parts):
    """the fixed 64-bit seed of a case (both halves in use)"""
    h = 0x9E3779B97F4A7C15
    for p in parts:
        h = (h * 0x100000001B3 + int(p) + 1) & ((1 << 64) - 1)
    return h


# ------------------------------------------------------------------ kernel level: tile lists
def _regions(tq, axis):
    """target regions (row0, col0, rows, cols, F_ROWS, source ld rule, destination ld rule, offset) of the
    type's matrix, as in test_gpu_fp4.py / test_gpu_fp6.py.  Along the block axis (length L) every op
    starts on a multiple of 32 and ends on one or at the matrix edge, where the last MX block is partial.
    The list holds whole 64 x 64 sub-tiles on aligned sides (FULL path), guarded remainders along f and
    along s, ops with row0 and col0 != 0.  ld rules: 'v' a multiple of 32, 'b' the matrix's row count (odd,
    2 mod 4 or 4 mod 8 by the type); the last op's sides start one packing group in."""
    M, N = DIMS[tq]
    L, O = (M, N) if axis == ROWS else (N, M)
    w0, w1, w2 = {1: (45, 31, 19), 2: (46, 30, 18), 4: (44, 28, 20)}[GROUP[tq]]
    reg = [
        (0, 0, 64, 64, True, "v", "v", 0),            # one whole sub-tile, blocks along f (FULL path)
        (64, 0, 64, 64, False, "v", "v", 0),          # one whole sub-tile, blocks along s (FULL path)
        (128, 0, L - 128, w0, True, "b", "v", 0),     # up to the edge along f: a partial block
        (128, w0, L - 128, w1, False, "v", "b", 0),   # the same with the blocks along s
        (0, 64, 96, O - 64, True, "b", "b", 0),       # remainder sub-tiles on both sides
        (96, 64, 32, w2, False, "v", "v", GROUP[tq]),  # aligned ld, the first element off the 16-byte grid
    ]
    return [(b0, o0, nb, no, along_f, sl, dl, off) if axis == ROWS else (o0, b0, no, nb, not along_f, sl, dl, off)
            for b0, o0, nb, no, along_f, sl, dl, off in reg]


def _tile_list(costa, tq, axis, transpose, kind):
    """-> (ops with ELEMENT offsets, source elements, destination elements)"""
    regions = _regions(tq, axis)
    ops = np.zeros(len(regions), costa.SCALED_OP_DTYPE)
    src_at = dst_at = 0
    for k, (r0, c0, nr, nc, frow, sl, dl, off) in enumerate(regions):
        nf, ns = (nr, nc) if frow else (nc, nr)

        def place(at, fast, slow, rule, off):
            ld = (fast + 31) // 32 * 32 if rule == "v" else DIMS[tq][0]
            assert ld >= fast
            return at + off, ld, (at + off + ld * slow + 31) // 32 * 32
        s0, lds, src_at = place(src_at, nf, ns, sl, off)
        df, dslow = (ns, nf) if transpose else (nf, ns)
        d0, ldd, dst_at = place(dst_at, df, dslow, dl, off)
        flags = (TR if transpose else 0) | kind << 4 | (F_ROWS if frow else 0)
        ops[k] = ((s0, d0, nf, ns, lds, ldd, flags, 0), r0, c0)
    return ops, src_at + 32, dst_at + 32


def _subtiles(ops):
    return sum(-(-int(o["op"]["nf"]) // 64) * -(-int(o["op"]["ns"]) // 64) for o in ops)


def _gpu_ops(ops, ta, tc):
    g = ops.copy()
    g["op"]["src"] = sr.byte_offset(ta, ops["op"]["src"])
    g["op"]["dst"] = sr.byte_offset(tc, ops["op"]["dst"])
    return g


def _sc_shape(m, n, axis):
    return (mc.n_blocks(m), n) if axis == ROWS else (mc.n_blocks(n), m)


def _tiles_model(costa, seed, ta, tc, transpose, a_axis, c_axis, rounding, alpha, kind):
    """the model half of a tile-list case (no GPU): inputs, expected outputs, the conditions"""
    m, n = DIMS[tc]
    ops, n_src, n_dst = _tile_list(costa, tc, c_axis, transpose, kind)
    a_tr = transpose and ta != F
    src = sr.source_data(ta, 0xA1, n_src)
    dst0 = sr.family(tc)[3](tc, 0xC1, n_dst)
    sa = None
    if ta != F:
        am, an = (n, m) if a_tr else (m, n)
        sa = mc.scale_bytes(0x5A, _sc_shape(am, an, a_axis))
    sc0 = np.full(_sc_shape(m, n, c_axis), 0xA5, np.uint8)
    what = (f"{NAMES[ta]}->{NAMES[tc]} {'tr' if transpose else 'copy'} axes {a_axis}->{c_axis} {RND[rounding]} "
            f"seed {seed:#x}")
    r = sr.expected_tiles_mx_sr(seed, ta, tc, ops, alpha, 0.0, src, dst0, m, n, sa=sa, a_axis=a_axis,
                                a_transposed=a_tr, c_axis=c_axis, rounding=rounding, sc_fill=sc0)
    _model_ok(r, tc, what)
    r.__dict__.update(ops=ops, src=src, dst0=dst0, sa=sa, sc0=sc0, a_tr=a_tr, what=what, m=m, n=n, alpha=alpha,
                      seed=seed, ta=ta, tc=tc, a_axis=a_axis, c_axis=c_axis, rounding=rounding)
    return r


def _tiles_gpu(costa, r, order):
    """run the SR call and the call without a seed on the same inputs; data against the model, the scale
    bytes against the model and against each other"""
    ta, tc, m, n = r.ta, r.tc, r.m, r.n
    scal = np.array([r.alpha, 0.0], np.float32)
    SA = ScaleT(costa, r.a_axis, *r.sa.shape, order, init=r.sa) if r.sa is not None else None
    ds = dev(r.src)
    out = {}
    for seed in (None, r.seed):
        SC = ScaleT(costa, r.c_axis, *r.sc0.shape, order)
        dd = dev(r.dst0)
        i0, s0 = costa.mx_items(), costa.scaled_items()
        costa.execute_tiles_mx(ta, tc, _gpu_ops(r.ops, ta, tc), scal, m, n, ds.data_ptr(), dd.data_ptr(),
                               a_scales=SA.desc if SA else None, c_scales=SC.desc, rounding=RND[r.rounding],
                               a_transposed=r.a_tr, stochastic_seed=seed)
        assert costa.mx_items() - i0 == _subtiles(r.ops) and costa.scaled_items() == s0
        SC.check(r.sc, r.what + f": c_scales (seed {seed})")
        out[seed] = (host(dd), SC.t.cpu().numpy())
    if SA:
        SA.check(SA.init, r.what + ": a_scales")
    same = sr.family(tc)[4]
    same(out[None][0], r.rn, tc, r.what + ": destination of the call without a seed")
    same(out[r.seed][0], r.exp, tc, r.what + ": destination")
    assert out[None][1].tobytes() == out[r.seed][1].tobytes(), r.what + ": scale bytes differ from the plain call's"
    assert ds.cpu().numpy().tobytes() == np.ascontiguousarray(r.src).view(np.uint8).tobytes()


def _rounding_of(transpose, axis):
    return CEIL if transpose != (axis == COLS) else FLOOR


QUANT_CASES = [(tq, transpose, axis) for tq in QTYPES for transpose in (False, True) for axis in (ROWS, COLS)]


def quantise_model(costa, tq, transpose, axis):
    kind, alpha = (ALPHA, -0.5) if transpose else (BITCOPY, 1.0)
    return _tiles_model(costa, _seed(1, tq, transpose, axis), F, tq, transpose, None, axis,
                        _rounding_of(transpose, axis), alpha, kind)


@pytest.mark.parametrize("tq,transpose,axis", QUANT_CASES,
                         ids=[f"{NAMES[t]}-{'tr' if tr else 'copy'}-{'rows' if a == ROWS else 'cols'}"
                              for t, tr, a in QUANT_CASES])
def test_quantise_tile_lists(costa, tq, transpose, axis):
    _tiles_gpu(costa, quantise_model(costa, tq, transpose, axis), "block" if axis == ROWS else "line")


REQUANT_CASES = [(tq, axes) for tq in (E4M3, FP4, E2M3) for axes in ((ROWS, COLS), (COLS, COLS))]


def requantise_model(costa, tq, axes):
    return _tiles_model(costa, _seed(2, tq, *axes), tq, tq, True, axes[0], axes[1], FLOOR, 0.625, ALPHA)


@pytest.mark.parametrize("tq,axes", REQUANT_CASES,
                         ids=[f"{NAMES[t]}-{'rows' if a[0] == ROWS else 'cols'}-cols" for t, a in REQUANT_CASES])
def test_requantise_tile_lists(costa, tq, axes):
    """'T': A's blocks along its rows or columns, C's along its columns; every block is cut anew"""
    _tiles_gpu(costa, requantise_model(costa, tq, axes), "line")


# ------------------------------------------------------------------ specials
def _special_matrix(tq):
    if tq in (E4M3, E5M2):
        from test_gpu_mx import _special_blocks
        return _special_blocks(tq)
    if tq == FP4:
        from test_gpu_fp4 import _special_blocks
        return _special_blocks()
    from test_gpu_fp6 import _special_blocks
    return _special_blocks(tq)


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("frow", [True, False], ids=["along-f", "along-s"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@TYPES
def test_special_blocks(costa, tq, transpose, frow, rounding):
    """the inf / NaN / zero / saturating blocks of the existing tests: blocks with E = 255 are stored as
    by the call without a seed, zero blocks are zeros with their signs, saturated elements are exactly
    the +-fmax code"""
    V = _special_matrix(tq)
    m, n = V.shape
    seed = _seed(3, tq, transpose, frow, rounding)
    src = (V.T if frow else V).reshape(-1).copy()  # element (f, s) at s * lds + f
    nf, ns = (m, n) if frow else (n, m)
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, nf, ns, nf, ns if transpose else nf, (TR if transpose else 0) | BITCOPY << 4 | (F_ROWS if frow else 0),
               0), 0, 0)
    what = f"specials {NAMES[tq]} {'tr' if transpose else 'copy'} frow {frow} {RND[rounding]}"
    dst0 = sr.family(tq)[3](tq, 0xC1, m * n)
    sc0 = np.full((1, n), 0xA5, np.uint8)
    r = sr.expected_tiles_mx_sr(seed, F, tq, ops, 1.0, 0.0, src, dst0, m, n, c_axis=ROWS, rounding=rounding, sc_fill=sc0)
    E = r.sc[0]
    assert (E == 255).sum() == 2 and (E == 0).sum() >= 2
    ds = dev(src)
    got = {}
    for s in (None, seed):
        SC = ScaleT(costa, ROWS, 1, n, "block")
        dd = dev(dst0)
        costa.execute_tiles_mx(F, tq, _gpu_ops(ops, F, tq), [1.0, 0.0], m, n, ds.data_ptr(), dd.data_ptr(),
                               c_scales=SC.desc, rounding=RND[rounding], stochastic_seed=s)
        SC.check(r.sc, what + f": c_scales (seed {s})")
        got[s] = host(dd)
    sr.family(tq)[4](got[seed], r.exp, tq, what)
    # the codes of the target matrix, whatever the destination's orientation
    def dense(buf):
        codes = sr.unpack(buf, tq).reshape((m, n) if transpose == frow else (n, m))
        return codes if transpose == frow else codes.T
    Q, R = dense(got[seed]), dense(got[None])
    nan_blocks = np.flatnonzero(E == 255)
    assert (Q[:, nan_blocks] == R[:, nan_blocks]).all()                # E = 255: as the call without a seed
    if tq in (E4M3, E5M2):
        assert np.isnan(sr.widen_codes(Q[:, nan_blocks], tq)).all()
        assert int(np.isnan(sr.widen_codes(Q, tq)).sum()) == 32 * nan_blocks.size
    else:
        assert (Q[:, nan_blocks] == 0).all()
    zero = np.flatnonzero((V == 0).all(axis=0))                        # zero blocks: zeros with their signs
    assert zero.size >= 1 and (E[zero] == 0).all()
    assert (Q[:, zero] == np.where(np.signbit(V[:, zero]), sr.SIGN[tq], 0)).all()
    assert (Q[:, zero] & sr.SIGN[tq]).any()
    with np.errstate(invalid="ignore"):
        sat = np.abs(r.t_pre) >= sr.FMAX[tq]                           # at or above fmax before the clamp
    top = sr.mags(tq).size - 1
    assert (Q[sat] == np.where(np.signbit(r.t_pre[sat]), top | sr.SIGN[tq], top)).all()
    if rounding == FLOOR:
        with np.errstate(invalid="ignore"):
            assert (np.abs(r.t_pre) > sr.FMAX[tq]).any(), what        # the clamp ran
    # elsewhere the seed matters: some finite element differs from the round-to-nearest call
    assert (Q != R).any()


# ------------------------------------------------------------------ transform_mx on one rank
def _geometry(tq, name, op, grid=(1, 1)):
    if tq == FP4:
        return f4.geometry(name, op, grid)
    if tq in f6.FP6:
        return f6.geometry(name, op, grid)
    return mc.geometry(name, op, grid)


def _scales_for(costa, case_shape, axis, order, init=None, fill=0xA5):
    shape = _sc_shape(*case_shape, axis)
    return ScaleT(costa, axis, *shape, order, init=None if init is None else init, fill=fill)


def _xf_model(seed, kind, tq, geom, op, a_axis, c_axis, rounding, alpha):
    ta = F if kind == "quantise" else tq
    a_case, c_case = _geometry(tq, geom, op)
    na, nc = a_case.buf_elems(0, 1), c_case.buf_elems(0, 1)
    a = sr.source_data(ta, 0x31, na)
    c = sr.family(tq)[3](tq, 0x33, nc)
    sa = mc.scale_bytes(0x34, _sc_shape(*a_case.shape(), a_axis)) if ta != F else None
    what = f"{kind} {NAMES[ta]}->{NAMES[tq]} {geom} {op} seed {seed:#x}"
    r = sr.expected_transform_mx_sr(seed, ta, tq, op, alpha, 0.0, a_case, c_case, 1, [a], [c], sa=sa, a_axis=a_axis,
                                    c_axis=c_axis, rounding=rounding)
    _model_ok(r, tq, what)
    r.__dict__.update(ta=ta, tc=tq, a_case=a_case, c_case=c_case, a=a, c=c, sa=sa, what=what, op=op, alpha=alpha,
                      a_axis=a_axis, c_axis=c_axis, rounding=rounding, seed=seed)
    return r


def _xf_gpu(costa, r, order="block", stream=None):
    ta, tc = r.ta, r.tc
    lay = sr.family(tc)[2]
    da, dc = dev(r.a), dev(r.c)
    SA = _scales_for(costa, r.a_case.shape(), r.a_axis, order, init=r.sa) if r.sa is not None else None
    SC = _scales_for(costa, r.c_case.shape(), r.c_axis, order)
    A = lay(costa, r.a_case, 0, da.data_ptr(), 1, ta)
    C = lay(costa, r.c_case, 0, dc.data_ptr(), 1, tc)
    i0 = costa.mx_items()
    costa.transform_mx(A, C, costa.Comm.self(0), r.op, r.alpha, 0.0, a_scales=SA.desc if SA else None,
                       c_scales=SC.desc, rounding=RND[r.rounding], stream=stream, stochastic_seed=r.seed)
    if stream is not None:
        stream.synchronize()
    SC.check(r.sc, r.what + ": c_scales")
    if SA:
        SA.check(SA.init, r.what + ": a_scales")
    sr.family(tc)[4](host(dc), r.exp[0], tc, r.what)
    assert da.cpu().numpy().tobytes() == np.ascontiguousarray(r.a).view(np.uint8).tobytes()
    assert costa.mx_items() > i0


# (type, geometry, op) of the one-rank cases: the four FP8 geometries, and one aligned and one custom
# geometry of each packed type
XF_GEOMS = [(E4M3, "g192", "N"), (E5M2, "g203", "T"), (E4M3, "g203pad", "T"), (E5M2, "custom32", "N"),
            (FP4, "g202", "T"), (FP4, "custom32", "N"), (E2M3, "g204", "T"), (E3M2, "custom32q", "N")]
XF_CASES = [(kind, tq, geom, op) for kind in ("quantise", "requantise") for tq, geom, op in XF_GEOMS]


def xf_model(kind, tq, geom, op):
    rounding = CEIL if geom.endswith("pad") else FLOOR
    # requantise 'T' turns the block axis round ('N' keeps it); the others alternate with the geometry
    a_axis = ROWS if geom in ("g192", "custom32", "custom32q") else COLS
    c_axis = (COLS if a_axis == ROWS else ROWS) if kind == "requantise" and op == "T" else a_axis
    alpha = 1.0 if op == "N" and kind == "quantise" else 0.625
    return _xf_model(_seed(4, kind == "quantise", tq, len(geom), op == "N"), kind, tq, geom, op, a_axis, c_axis,
                     rounding, alpha)


@pytest.mark.parametrize("kind,tq,geom,op", XF_CASES, ids=[f"{k}-{NAMES[t]}-{g}-{o}" for k, t, g, o in XF_CASES])
def test_transform_mx_one_rank(costa, kind, tq, geom, op):
    _xf_gpu(costa, xf_model(kind, tq, geom, op), order="block" if op == "N" else "line")


def async_model():
    return _xf_model(_seed(5), "quantise", E4M3, "g203", "T", ROWS, COLS, FLOOR, 0.75)


def test_transform_mx_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _xf_gpu(costa, async_model(), stream=s)


# ------------------------------------------------------------------ invariance
def _dense_codes(tq, case, buf):
    """the dense matrix of a rank's C buffer, as fp32 bit patterns (one per code, -0 kept)"""
    return mc.gather(case, 1, [sr.widen(buf, tq)]).view(np.uint32)


def _run_dense(costa, tq, a_case, c_case, op, X, seed, axis):
    """quantise the dense fp32 matrix X (A's matrix as stored) -> (dense codes of C, its scale bytes)"""
    lay = sr.family(tq)[2]
    a = mc.place(a_case, 1, X, [np.zeros(a_case.buf_elems(0, 1), np.float32)])[0]
    c = sr.family(tq)[3](tq, 0x35, c_case.buf_elems(0, 1))
    da, dc = dev(a), dev(c)
    SC = _scales_for(costa, c_case.shape(), axis, "block")
    costa.transform_mx(lay(costa, a_case, 0, da.data_ptr(), 1, F), lay(costa, c_case, 0, dc.data_ptr(), 1, tq),
                       costa.Comm.self(0), op, 0.75, 0.0, c_scales=SC.desc, stochastic_seed=seed)
    return _dense_codes(tq, c_case, host(dc)), SC.t.cpu().numpy()[SC.at]


def invariance_model(tq):
    """the dense 200 x 170 input and what the model says about it"""
    from casegen import BC
    m, n = 200, 170
    X = mc.quant_data(0x41, m * n).reshape(m, n)
    seed = _seed(6, tq)
    c_bc = BC(m, n, 96, 32)
    a_bc = BC(m, n, 64, 64)
    c0 = sr.family(tq)[3](tq, 0x35, c_bc.buf_elems(0, 1))
    a = mc.place(a_bc, 1, X, [np.zeros(a_bc.buf_elems(0, 1), np.float32)])
    r = sr.expected_transform_mx_sr(seed, F, tq, "N", 0.75, 0.0, a_bc, c_bc, 1, a, [c0], c_axis=COLS)
    _model_ok(r, tq, f"invariance {NAMES[tq]}")
    r.__dict__.update(X=X, seed=seed, a_bc=a_bc, c_bc=c_bc)
    return r


@pytest.mark.parametrize("tq", [E4M3, FP4], ids=["e4m3", "e2m1"])
def test_layouts_and_op_do_not_change_the_codes(costa, tq):
    """the same dense input and seed through two C layouts (block-cyclic 96 x 32 blocks, the custom32
    cuts), and 'N' from A against 'T' from the transposed A: one dense code matrix, the model's"""
    r = invariance_model(tq)
    m, n = r.X.shape
    custom_a, custom_c = _geometry(tq, "custom32", "N")
    custom_at, _ = _geometry(tq, "custom32", "T")
    assert custom_c.shape() == (m, n)
    want = sr.widen_codes(r.q, tq).view(np.uint32)
    runs = {"BC 96x32 'N'": _run_dense(costa, tq, r.a_bc, r.c_bc, "N", r.X, r.seed, COLS),
            "custom32 'N'": _run_dense(costa, tq, custom_a, custom_c, "N", r.X, r.seed, COLS),
            "custom32 'T'": _run_dense(costa, tq, custom_at, custom_c, "T", np.ascontiguousarray(r.X.T), r.seed, COLS)}
    for name, (codes, sc) in runs.items():
        assert codes.shape == want.shape and (codes == want).all(), f"{NAMES[tq]} {name}: dense codes differ"
        assert sc.tobytes() == r.sc.tobytes(), f"{NAMES[tq]} {name}: scale bytes differ"


# ------------------------------------------------------------------ seeds
def seeds_model(tq):
    s = _seed(7, tq) & ~(1 << 32)
    geom, op = ("g203", "T") if tq == E4M3 else ("g202", "T")
    return [_xf_model(x, "quantise", tq, geom, op, ROWS, COLS, FLOOR, 0.75) for x in (s, s + 1, s + (1 << 32))]


@pytest.mark.parametrize("tq", [E4M3, FP4], ids=["e4m3", "e2m1"])
def test_seeds(costa, tq):
    """the same seed twice: identical bytes; s and s + 1, s and s + 2^32: other data, the same scale bytes;
    the seed is no part of the plan (no plan-cache miss after the pair's first call); mx_items counts"""
    rs = seeds_model(tq)
    r = rs[0]
    lay = sr.family(tq)[2]
    da, dc = dev(r.a), dev(r.c)
    A = lay(costa, r.a_case, 0, da.data_ptr(), 1, F)
    C = lay(costa, r.c_case, 0, dc.data_ptr(), 1, tq)
    comm = costa.Comm.self(0)

    def run(seed):
        dc.copy_(dev(r.c))
        SC = _scales_for(costa, r.c_case.shape(), COLS, "line")
        costa.transform_mx(A, C, comm, "T", 0.75, 0.0, c_scales=SC.desc, stochastic_seed=seed)
        SC.check(r.sc, f"seed {seed}: c_scales")
        return host(dc).tobytes()
    plain = run(None)                                                  # the pair's plan exists from here on
    st0, i0 = costa.get_stats(), costa.mx_items()
    got = [run(x.seed) for x in rs]
    again = run(r.seed)
    st1 = costa.get_stats()
    assert st1["plan_misses"] == st0["plan_misses"] and st1["plan_hits"] - st0["plan_hits"] == 4
    assert costa.mx_items() > i0
    assert again == got[0]
    for x, g in zip(rs, got):
        sr.family(tq)[4](np.frombuffer(g, np.uint8), x.exp[0], tq, x.what)
    assert got[0] != got[1] and got[0] != got[2] and got[1] != got[2] and plain not in got
    assert run(None) == plain


# ------------------------------------------------------------------ several ranks on one GPU
def ranks_model(tq, op):
    P = 4
    geom = "g203" if tq == E4M3 else "g202"
    a_case, c_case = _geometry(tq, geom, op, (2, 2))
    a = [mc.quant_data(0x40 + r, a_case.buf_elems(r, P)) for r in range(P)]
    c = [sr.family(tq)[3](tq, 0x50 + r, c_case.buf_elems(r, P)) for r in range(P)]
    axis = COLS if op == "T" else ROWS
    seed = _seed(8, tq, op == "T")
    r = sr.expected_transform_mx_sr(seed, F, tq, op, 0.75, 0.0, a_case, c_case, P, a, c, c_axis=axis)
    _model_ok(r, tq, f"ranks {NAMES[tq]} {op}")
    r.__dict__.update(a_case=a_case, c_case=c_case, a=a, c=c, axis=axis, seed=seed, P=P)
    return r


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("tq", [E4M3, FP4], ids=["e4m3", "e2m1"])
def test_emulated_ranks_2x2(costa, tq, op):
    """quantise on 2 x 2 ranks (fp32 packages, quantised by UNPACK and LOCAL): every rank's buffer equals
    the GLOBAL model, whose random bits are keyed on C's coordinates; each rank's c_scales holds exactly
    its own blocks' bytes over a zero fill and their maximum is the model's tensor"""
    r = ranks_model(tq, op)
    P, a_case, c_case, axis = r.P, r.a_case, r.c_case, r.axis
    lay = sr.family(tq)[2]
    da, dc = [dev(x) for x in r.a], [dev(x) for x in r.c]
    L = [(lay(costa, a_case, k, da[k].data_ptr(), P, F), lay(costa, c_case, k, dc[k].data_ptr(), P, tq))
         for k in range(P)]
    plans = [costa.plan_export_scaled(L[k][0], L[k][1], k, P, op, 0.75, 0.0) for k in range(P)]
    assert all(p.send_elems > 0 and p.recv_elems > 0 for p in plans)
    sc_shape = _sc_shape(*c_case.shape(), axis)
    SC = [ScaleT(costa, axis, *sc_shape, "block", fill=0) for _ in range(P)]
    i0, s0 = costa.mx_items(), costa.scaled_items()

    def call(k, comm):
        costa.transform_mx(L[k][0], L[k][1], comm, op, 0.75, 0.0, c_scales=SC[k].desc, stochastic_seed=r.seed)

    out = drive(costa, plans, 4, call)
    assert out.stats["pack_launches"] > 0 and out.stats["unpack_launches"] > 0
    assert costa.mx_items() > i0 and costa.scaled_items() == s0
    for k in range(P):
        sr.family(tq)[4](host(dc[k]), r.exp[k], tq, f"quantise {NAMES[tq]} {op} rank {k}")
    merged = np.zeros(sc_shape, np.uint8)
    n_own = 0
    for k in range(P):
        own = mc.owned(c_case, P, k)
        first = (own if axis == ROWS else own.T)[::32, :]   # the rank owns a block with its first element
        mine = np.where(first, r.sc, 0).astype(np.uint8)
        SC[k].check(mine, f"quantise {op} rank {k}: c_scales")
        merged = np.maximum(merged, mine)
        n_own += int(first.sum())
    assert n_own == r.sc.size and merged.tobytes() == r.sc.tobytes()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_mx_sr_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK on the SR instances (tests/mx_sr_loopback_child.py)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mx_sr_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    p = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = p.stdout.strip().splitlines()
    assert p.returncode == 0 and out and out[-1].startswith("OK"), p.stdout + p.stderr
    _, n, packs, unpacks, locals_ = out[-1].split()
    assert int(n) == 3 and int(packs) > 0 and int(unpacks) > 0, out[-1]
    assert (int(locals_) == 0) == (mode == "1"), out[-1]


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_unchanged(costa):
    comm = costa.Comm.self(0)
    a_case, c_case = mc.geometry("g192", "N")
    m, n = c_case.shape()
    na = a_case.buf_elems(0, 1)
    data = {F: mc.quant_data(1, na), E4M3: sr.source_data(E4M3, 2, na)}
    sc0 = np.full((mc.n_blocks(m), n), 0x5A, np.uint8)
    dsa, dsc = dev(sc0), dev(sc0)
    SA = costa.mx_scales(dsa.view(mc.n_blocks(m), n), "rows")
    SC = costa.mx_scales(dsc.view(mc.n_blocks(m), n), "rows")

    def refused(ta, tc, match, a_scales, c_scales, beta=0.0, cases=(a_case, c_case), seed=7):
        c0 = np.resize(np.arange(251, dtype=np.uint8), cases[1].buf_elems(0, 1) * 4)
        da, dc = dev(np.resize(data[ta].view(np.uint8), cases[0].buf_elems(0, 1) * 4)), dev(c0)
        with pytest.raises(costa.CostaError, match=match) as e:
            costa.transform_mx(mc.make_layout(costa, cases[0], 0, da.data_ptr(), 1, ta),
                               mc.make_layout(costa, cases[1], 0, dc.data_ptr(), 1, tc), comm, "N", 1.0, beta,
                               a_scales=a_scales, c_scales=c_scales, stochastic_seed=seed)
        assert e.value.code == 1, str(e.value)
        assert dc.cpu().numpy().tobytes() == c0.tobytes()
        assert dsa.cpu().numpy().tobytes() == sc0.tobytes() and dsc.cpu().numpy().tobytes() == sc0.tobytes()
        return str(e.value)

    # a dequantise pair with a seed; without one the same call is accepted (checked at the end)
    msg = refused(E4M3, F, "stochastic rounding", SA, None)
    assert "FP8_E4M3" in msg and "FLOAT" in msg
    refused(E4M3, F, "stochastic rounding", SA, None, beta=2.0)
    # the checks of the plain call come first, with its messages
    refused(F, E4M3, "beta must be 0", None, SC, beta=2.0)
    refused(E4M3, E4M3, "beta must be 0", SA, SC, beta=-1.0)
    refused(F, E4M3, "c_scales is required", None, None)
    refused(E4M3, E4M3, "a_scales is required", None, SC)
    refused(E4M3, F, "a_scales is required", None, None)
    refused(F, F, "no MX transform", None, None)
    bc = mc.geometry("bc203", "N")
    m2, n2 = bc[1].shape()
    big = dev(np.full(max(m2, n2) * 8, 0x5A, np.uint8))
    for axis, shape in ((ROWS, (mc.n_blocks(m2), n2)), (COLS, (mc.n_blocks(n2), m2))):
        refused(F, E4M3, "MX block", None, costa.MxScales(big.data_ptr(), axis, shape[1], 1), cases=bc)
    assert big.cpu().numpy().tobytes() == bytes([0x5A]) * (max(m2, n2) * 8)
    # tile lists: a dequantise list with a seed, a split block, beta != 0
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ops[0] = ((0, 0, 32, 8, 32, 32, ALPHA << 4 | F_ROWS, 0), 0, 0)
    dd, src = dev(np.zeros(4096, np.uint8)), dev(data[E4M3])
    with pytest.raises(costa.CostaError, match="stochastic rounding"):
        costa.execute_tiles_mx(E4M3, F, ops, [1, 0], 64, 8, src.data_ptr(), dd.data_ptr(), a_scales=SA, stochastic_seed=3)
    ops["op"]["nf"] = 40
    with pytest.raises(costa.CostaError, match="MX block"):
        costa.execute_tiles_mx(F, E4M3, ops, [1, 0], 64, 8, dev(data[F]).data_ptr(), dd.data_ptr(), c_scales=SC,
                               stochastic_seed=3)
    ops["op"]["nf"], ops["op"]["flags"] = 32, AXPBY << 4 | F_ROWS
    with pytest.raises(costa.CostaError, match="beta must be 0"):
        costa.execute_tiles_mx(F, E4M3, ops, [1, 2], 64, 8, dev(data[F]).data_ptr(), dd.data_ptr(), c_scales=SC,
                               stochastic_seed=3)
    assert not dd.cpu().numpy().any() and dsc.cpu().numpy().tobytes() == sc0.tobytes()
    # the Python check of the seed: before anything reaches the library
    da, dc = dev(data[F]), dev(np.zeros(c_case.buf_elems(0, 1), np.uint8))
    for bad in (-1, 1 << 64, 1.5):
        with pytest.raises(ValueError):
            costa.transform_mx(mc.make_layout(costa, a_case, 0, da.data_ptr(), 1, F),
                               mc.make_layout(costa, c_case, 0, dc.data_ptr(), 1, E4M3), comm, c_scales=SC,
                               stochastic_seed=bad)
        with pytest.raises(ValueError):
            costa.execute_tiles_mx(F, E4M3, ops, [1, 0], 64, 8, da.data_ptr(), dd.data_ptr(), c_scales=SC,
                                   stochastic_seed=bad)
    assert not dc.cpu().numpy().any() and dsc.cpu().numpy().tobytes() == sc0.tobytes()
    # and the calls work afterwards: the dequantise without a seed, a quantise with one
    dq, dout = dev(data[E4M3]), dev(np.zeros(c_case.buf_elems(0, 1), np.float32))
    costa.transform_mx(mc.make_layout(costa, a_case, 0, dq.data_ptr(), 1, E4M3),
                       mc.make_layout(costa, c_case, 0, dout.data_ptr(), 1, F), comm, a_scales=SA)
    assert dout.cpu().numpy().any()
    _xf_gpu(costa, xf_model("quantise", E4M3, "g192", "N"))


# ------------------------------------------------------------------ neighbours
def test_plain_mx_calls_are_unchanged_around_sr_calls(costa):
    """transform_mx without a seed on the same layout handles gives identical bytes before and after SR
    calls: quantise and requantise, data and scale bytes"""
    rq = _xf_model(_seed(9), "requantise", E4M3, "g203", "T", ROWS, COLS, FLOOR, 0.625)
    qu = _xf_model(_seed(10), "quantise", E2M3, "g204", "T", ROWS, COLS, CEIL, 0.75)
    comm = costa.Comm.self(0)
    state = []
    for r in (rq, qu):
        lay = sr.family(r.tc)[2]
        da, dc = dev(r.a), dev(r.c)
        dsa = dev(r.sa).view(r.sa.shape) if r.sa is not None else None
        dsc = torch.zeros(*_sc_shape(*r.c_case.shape(), COLS), dtype=torch.uint8, device="cuda")
        state.append((r, lay(costa, r.a_case, 0, da.data_ptr(), 1, r.ta), lay(costa, r.c_case, 0, dc.data_ptr(), 1, r.tc),
                      da, dc, dsa, dsc))

    def call(k, seed):
        r, A, C, da, dc, dsa, dsc = state[k]
        dc.copy_(dev(r.c))
        dsc.zero_()
        costa.transform_mx(A, C, comm, "T", r.alpha, 0.0,
                           a_scales=costa.mx_scales(dsa, r.a_axis, r.a_case.shape()) if dsa is not None else None,
                           c_scales=costa.mx_scales(dsc, COLS, r.c_case.shape()), rounding=RND[r.rounding],
                           stochastic_seed=seed)
        return host(dc).tobytes(), dsc.cpu().numpy().tobytes()
    before = [call(k, None) for k in range(2)]
    for k in range(2):
        r = state[k][0]
        assert before[k][0] == np.ascontiguousarray(r.rn[0]).view(np.uint8).tobytes() and before[k][1] == r.sc.tobytes()
    i0 = costa.mx_items()
    for k in range(2):
        r = state[k][0]
        data, scales = call(k, r.seed)
        sr.family(r.tc)[4](np.frombuffer(data, np.uint8), r.exp[0], r.tc, r.what)
        assert scales == before[k][1] and data != before[k][0]
    assert costa.mx_items() > i0
    assert [call(k, None) for k in range(2)] == before
