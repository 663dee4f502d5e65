"""Dual-output MX quantise on the GPU (costa_hip.h, "Dual-output MX quantise"): mx_dual_kernel through
costa_hip_execute_tiles_mx_dual, and costa_hip_transform_mx_dual on one rank, on a stream, on emulated
ranks and through the loopback exchange.  Every expected byte comes from the CPU models of the MX tests
applied twice (mx_dual_common.py): once to op(A) for C, once to op(A)^T for Ct.  Comparison is exact: data
bytes, scale bytes and every byte around them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mx_common as mc
import mx_dual_common as dc
import mx_sr_common as sr
from emulated_ranks import drive
from mx_dual_common import E2M3, E3M2, E4M3, E5M2, F, FP4, GEOM_IDS, GEOMS, NAMES, OTHER, QTYPES
from mx_sr_common import CEIL, COLS, FLOOR, ROWS
from test_gpu_mx import ScaleT, dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR, F_ROWS = 0x1, 0x80
BITCOPY, ALPHA, AXPBY = 0, 2, 3
RND = {FLOOR: "floor", CEIL: "ceil"}
TYPES = pytest.mark.parametrize("tq", QTYPES, ids=[NAMES[t] for t in QTYPES])
GROUP = {E4M3: 1, E5M2: 1, FP4: 2, E2M3: 4, E3M2: 4}
SEED = 0x0123456789ABCDEF
MODES = [(False, False), (False, True), (True, False), (True, True)]
MODE_IDS = ["copy-copy", "copy-tr", "tr-copy", "tr-tr"]
AXES = [(ROWS, ROWS), (ROWS, COLS), (COLS, ROWS), (COLS, COLS)]
AXES_IDS = ["rows-rows", "rows-cols", "cols-rows", "cols-cols"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def host(t):
    return t.cpu().numpy().view(np.uint8)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


# ------------------------------------------------------------------ kernel level: tile lists
def _dims(tq):
    """205 x 120 for FP8 (partial blocks of 13 and 24 at the edges), 204 x 120 for the packed types"""
    return (205, 120) if GROUP[tq] == 1 else (204, 120)


def _regions(tq):
    """(row0, col0, rows, cols, F_ROWS, source / dst / dst2 offset in elements): every region starts on
    multiples of 32 in both dimensions and ends on one or at the edge"""
    M, N = _dims(tq)
    odd = {1: 3, 2: 2, 4: 4}[GROUP[tq]]  # off the side's strip alignment, whole packing groups
    return [
        (0, 0, 64, 64, True, 0, 0, 0),           # one whole 64 x 64: the FULL path
        (64, 0, 96, 32, False, 0, 0, 0),         # 96 x 32: partial sub-tiles
        (160, 0, 32, 32, True, 0, 0, 0),         # 32 x 32
        (192, 0, M - 192, 64, False, 0, 0, 0),   # the bottom edge strip (13 / 12 rows)
        (0, 96, 64, N - 96, True, 0, 0, 0),      # the right edge strip (24 columns)
        (64, 32, 64, 32, True, 1, 0, 0),         # odd source offset: VEC_SRC clear
        (64, 64, 64, 32, False, 0, odd, 0),      # odd dst offset: VEC_DST clear
        (128, 64, 64, N - 64, True, 0, 0, odd),  # odd dst2 offset: output 2's VEC_DST clear
        (0, 64, 64, 32, False, 0, 0, 0),         # a second whole-block op with the blocks the other way
    ]


def _tile_list(costa, tq, tr1, tr2, kind):
    """-> (dual ops with ELEMENT offsets, source / dst / dst2 elements)"""
    regions = _regions(tq)
    ops = np.zeros(len(regions), costa.DUAL_OP_DTYPE)
    at = [0, 0, 0]
    for k, (r0, c0, nr, nc, frow, so, do, d2o) in enumerate(regions):
        nf, ns = (nr, nc) if frow else (nc, nr)

        def place(which, fast, slow, off):
            ld = (fast + 15) // 16 * 16 + (4 if off else 0)
            first = at[which] + off
            at[which] = (first + ld * slow + 31) // 32 * 32
            return first, ld
        s0, lds = place(0, nf, ns, so)
        d0, ldd = place(1, *((ns, nf) if tr1 else (nf, ns)), do)
        d20, ldd2 = place(2, *((ns, nf) if tr2 else (nf, ns)), d2o)
        flags = (TR if tr1 else 0) | kind << 4 | (F_ROWS if frow else 0)
        ops[k] = (((s0, d0, nf, ns, lds, ldd, flags, 0), r0, c0), d20, ldd2, TR if tr2 else 0)
    return ops, at[0] + 32, at[1] + 32, at[2] + 32


def _subtiles(ops):
    return sum(-(-int(o["s"]["op"]["nf"]) // 64) * -(-int(o["s"]["op"]["ns"]) // 64) for o in ops)


def _gpu_ops(ops, tq, bases=(0, 0, 0)):
    g = ops.copy()
    g["s"]["op"]["src"] = ops["s"]["op"]["src"] * 4 + bases[0]
    g["s"]["op"]["dst"] = sr.byte_offset(tq, ops["s"]["op"]["dst"]) + bases[1]
    g["dst2"] = sr.byte_offset(tq, ops["dst2"]) + bases[2]
    return g


def _run_tiles(costa, tq, tr1, tr2, c_axis, ct_axis, order, rounding, alpha, seed=None, absolute=False, src=None,
               lst=None, dims=None):
    what = (f"dual tiles {NAMES[tq]} {'tr' if tr1 else 'copy'}/{'tr' if tr2 else 'copy'} axes {c_axis}/{ct_axis} "
            f"{order} {RND[rounding]} alpha {alpha} seed {seed}")
    m, n = dims or _dims(tq)
    kind = BITCOPY if alpha == 1.0 else ALPHA
    ops, n_src, n_dst, n_dst2 = lst or _tile_list(costa, tq, tr1, tr2, kind)
    if src is None:
        src = mc.quant_data(0xA1, n_src)
    fill = sr.family(tq)[3]
    dst0, dst20 = fill(tq, 0xC1, n_dst), fill(tq, 0xC2, n_dst2)
    SC = ScaleT(costa, c_axis, *dc.sc_shape(m, n, c_axis), order)
    SCt = ScaleT(costa, ct_axis, *dc.sc_shape(n, m, ct_axis), "line" if order == "block" else "block", fill=0x3C)
    (e1, s1, t1), (e2, s2, t2) = dc.expected_tiles(tq, ops, alpha, src, dst0, dst20, m, n, c_axis, ct_axis, rounding,
                                                   SC.init, SCt.init, seed)
    if np.isfinite(src).all():
        dc.assert_finite([e1, e2], tq, what)
    ds, dd, dd2 = dev(src), dev(dst0), dev(dst20)
    i0, x0, s0, a0 = costa.mx_dual_items(), costa.mx_items(), costa.scaled_items(), costa.amax_items()
    scal = np.array([alpha, 0.0], np.float32)
    if absolute:
        costa.execute_tiles_mx_dual(tq, _gpu_ops(ops, tq, (ds.data_ptr(), dd.data_ptr(), dd2.data_ptr())), scal, m, n,
                                    c_scales=SC.desc, ct_scales=SCt.desc, rounding=RND[rounding], stochastic_seed=seed)
    else:
        costa.execute_tiles_mx_dual(tq, _gpu_ops(ops, tq), scal, m, n, ds.data_ptr(), dd.data_ptr(), dd2.data_ptr(),
                                    c_scales=SC.desc, ct_scales=SCt.desc, rounding=RND[rounding], stochastic_seed=seed)
    SC.check(s1, what + ": c_scales")
    SCt.check(s2, what + ": ct_scales")
    same = sr.family(tq)[4]
    same(host(dd), e1, tq, what + ": output 1")
    same(host(dd2), e2, tq, what + ": output 2")
    assert costa.mx_dual_items() - i0 == _subtiles(ops)
    assert costa.mx_items() == x0 and costa.scaled_items() == s0 and costa.amax_items() == a0
    assert host(ds).tobytes() == raw(src)
    return (host(dd), e1, s1, t1), (host(dd2), e2, s2, t2), (SC, SCt)


@pytest.mark.parametrize("axes", AXES, ids=AXES_IDS)
@pytest.mark.parametrize("modes", MODES, ids=MODE_IDS)
@TYPES
def test_dual_tile_lists(costa, tq, modes, axes):
    """the five types x the four output modes x the four axis combinations; the tensors' storage, the
    rounding rule and alpha (1: BITCOPY, -0.5: ALPHA) alternate so that each value meets each mode and axis"""
    k = MODES.index(modes) + AXES.index(axes)
    order = "block" if k % 2 == 0 else "line"
    rounding = FLOOR if (k // 2 + QTYPES.index(tq)) % 2 == 0 else CEIL
    alpha = 1.0 if (k + QTYPES.index(tq)) % 3 else -0.5
    o1, o2, _ = _run_tiles(costa, tq, *modes, *axes, order, rounding, alpha)
    if GROUP[tq] == 1:  # FP8: the clamp ran under floor (values above fmax before it, +-fmax stored), never under ceil
        fm = float(mc.FMAX[tq])
        for got, _, _, t in (o1, o2):
            if rounding == FLOOR:
                assert (np.abs(t) > fm).any() and (np.abs(mc.widen(got, tq)) == fm).any()
            else:
                assert (np.abs(t) <= fm).all()


@pytest.mark.parametrize("rounding", [FLOOR, CEIL], ids=["floor", "ceil"])
@pytest.mark.parametrize("order", ["block", "line"])
@pytest.mark.parametrize("alpha", [1.0, -0.5])
def test_dual_tile_lists_every_setting(costa, order, rounding, alpha):
    """block- and line-major tensors x floor and ceil x alpha 1 and -0.5 on one type and mode"""
    _run_tiles(costa, E4M3, False, True, ROWS, ROWS, order, rounding, alpha)


@TYPES
def test_dual_tile_lists_absolute_addresses(costa, tq):
    _run_tiles(costa, tq, True, False, COLS, ROWS, "line", FLOOR, -0.5, absolute=True)


@pytest.mark.parametrize("modes", MODES, ids=MODE_IDS)
@TYPES
def test_dual_tile_lists_sr(costa, tq, modes):
    """stochastic rounding: Ct keyed on (j, i); the scale bytes are those of the nearest call, and a
    second seed changes data bytes and no scale byte"""
    axes = AXES[(MODES.index(modes) + QTYPES.index(tq)) % 4]
    o1, o2, _ = _run_tiles(costa, tq, *modes, *axes, "block", FLOOR, -0.5, seed=SEED)
    n1, n2, _ = _run_tiles(costa, tq, *modes, *axes, "block", FLOOR, -0.5)
    p1, p2, _ = _run_tiles(costa, tq, *modes, *axes, "block", FLOOR, -0.5, seed=SEED ^ 0xFFFF0000FFFF)
    for a, b, c in ((o1, n1, p1), (o2, n2, p2)):
        assert a[2].tobytes() == b[2].tobytes() == c[2].tobytes()       # scale bytes
        assert a[0].tobytes() != b[0].tobytes() and a[0].tobytes() != c[0].tobytes()


@TYPES
def test_dual_specials(costa, tq):
    """one 64 x 64 matrix with a NaN, an inf, an all-zero block, an all-subnormal block and FLT_MAX: E = 255
    in exactly the blocks that hold the NaN or the inf -- different blocks in the two outputs, which are cut
    along different dimensions"""
    m = n = 64
    V = (np.random.default_rng(7).uniform(-1, 1, (m, n)) * 4).astype(np.float32)
    V[0:32, 5] = 0.0                                                    # an all-zero block of C
    V[32:64, 6] = np.float32(1e-42) * np.arange(1, 33, dtype=np.float32)  # an all-subnormal block
    V[40, 0:32] = 0.0                                                   # an all-zero block of Ct
    V[3, 10] = np.nan
    V[50, 40] = np.inf
    V[20, 50] = np.finfo(np.float32).max
    ops = np.zeros(1, costa.DUAL_OP_DTYPE)
    ops[0] = (((0, 0, m, n, m, m, BITCOPY << 4 | F_ROWS, 0), 0, 0), 0, n, TR)
    src = V.T.reshape(-1).copy()  # element (f, s) = V[f, s] at s * m + f
    (g1, e1, s1, _), (g2, e2, s2, _), _ = _run_tiles(costa, tq, False, True, ROWS, ROWS, "block", FLOOR, 1.0, src=src,
                                                     lst=(ops, m * n, m * n, m * n), dims=(m, n))
    # C: blocks of 32 rows per column; Ct = V^T: blocks of 32 of Ct's rows (V's columns) per Ct column (V's row)
    want1 = np.zeros((2, n), bool)
    want1[0, 10] = want1[1, 40] = True
    want2 = np.zeros((2, m), bool)
    want2[0, 3] = want2[1, 50] = True
    assert ((s1 == 255) == want1).all() and ((s2 == 255) == want2).all()
    assert s1[0, 5] == 0 and s1[1, 6] == 0 and s2[0, 40] == 0
    nan_code = sr.NAN_CODE[tq]
    c1, c2 = sr.unpack(g1, tq).reshape(n, m).T, sr.unpack(g2, tq).reshape(n, m)  # both as V[i, j]
    for c, rows, cols in ((c1, slice(0, 32), 10), (c1, slice(32, 64), 40), (c2, 3, slice(0, 32)), (c2, 50, slice(32, 64))):
        blk = c[rows, cols] & np.uint8(2 * sr.SIGN[tq] - 1 if GROUP[tq] > 1 else 0x7F)
        assert (blk == nan_code).all(), (NAMES[tq], blk)
    if GROUP[tq] == 1:
        assert np.isnan(mc.widen(g1, tq)).sum() == 64 and np.isnan(mc.widen(g2, tq)).sum() == 64


# ------------------------------------------------------------------ transform_mx_dual on one rank
def _case(tq, geom, op, ct_ord, grid=(1, 1)):
    a_case, c_case = dc.geometry(tq, geom, op, grid)
    return a_case, c_case, dc.twin(c_case, ct_ord)


class Run:
    """the inputs, device buffers, layouts and scale tensors of one dual transform on P ranks"""

    def __init__(self, costa, tq, cases, P=1, c_axis=ROWS, ct_axis=ROWS, order="block", sc_fill=0xA5):
        self.costa, self.tq, self.P = costa, tq, P
        self.a_case, self.c_case, self.ct_case = cases
        fill, lay = sr.family(tq)[3], sr.family(tq)[2]
        self.a = [mc.quant_data(0x31 + r, self.a_case.buf_elems(r, P)) for r in range(P)]
        self.c = [fill(tq, 0x41 + r, self.c_case.buf_elems(r, P)) for r in range(P)]
        self.ct = [fill(tq, 0x51 + r, self.ct_case.buf_elems(r, P)) for r in range(P)]
        self.da, self.dc, self.dct = [[dev(x) for x in v] for v in (self.a, self.c, self.ct)]
        self.A = [lay(costa, self.a_case, r, self.da[r].data_ptr(), P, F) for r in range(P)]
        self.C = [lay(costa, self.c_case, r, self.dc[r].data_ptr(), P, tq) for r in range(P)]
        self.Ct = [lay(costa, self.ct_case, r, self.dct[r].data_ptr(), P, tq) for r in range(P)]
        m, n = self.c_case.shape()
        self.c_axis, self.ct_axis = c_axis, ct_axis
        self.SC = [ScaleT(costa, c_axis, *dc.sc_shape(m, n, c_axis), order, fill=sc_fill) for _ in range(P)]
        self.SCt = [ScaleT(costa, ct_axis, *dc.sc_shape(n, m, ct_axis), order, fill=sc_fill) for _ in range(P)]

    def expected(self, op, alpha, rounding=FLOOR, seed=None):
        return dc.expected_transform(self.tq, op, alpha, self.a_case, self.c_case, self.ct_case, self.P, self.a, self.c,
                                     self.ct, self.c_axis, self.ct_axis, rounding, seed)

    def call(self, op, alpha, rounding=FLOOR, seed=None, stream=None, r=0, comm=None):
        self.costa.transform_mx_dual(self.A[r], self.C[r], self.Ct[r], comm or self.costa.Comm.self(0), op, alpha,
                                     c_scales=self.SC[r].desc, ct_scales=self.SCt[r].desc, rounding=RND[rounding],
                                     stochastic_seed=seed, stream=stream)

    def reset(self):
        for r in range(self.P):
            self.dc[r].copy_(dev(self.c[r]))
            self.dct[r].copy_(dev(self.ct[r]))
            self.SC[r].t.copy_(dev(self.SC[r].full0))
            self.SCt[r].t.copy_(dev(self.SCt[r].full0))

    def check_one_rank(self, exp, what):
        (e1, s1, _), (e2, s2, _) = exp
        dc.assert_finite(e1 + e2, self.tq, what)
        self.SC[0].check(s1, what + ": c_scales")
        self.SCt[0].check(s2, what + ": ct_scales")
        same = sr.family(self.tq)[4]
        same(host(self.dc[0]), e1[0], self.tq, what + ": C")
        same(host(self.dct[0]), e2[0], self.tq, what + ": Ct")
        assert host(self.da[0]).tobytes() == raw(self.a[0]), what + ": A changed"


@pytest.mark.parametrize("ct_ord", ["C", "R"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("tq,geom", GEOMS, ids=GEOM_IDS)
def test_transform_mx_dual_one_rank(costa, tq, geom, op, ct_ord):
    k = GEOM_IDS.index(f"{NAMES[tq]}-{geom}") + (op == "T") + 2 * (ct_ord == "R")
    c_axis, ct_axis = AXES[k % 4]
    rounding = CEIL if geom.endswith("pad") else FLOOR
    alpha = 1.0 if op == "N" else 0.75
    run = Run(costa, tq, _case(tq, geom, op, ct_ord), c_axis=c_axis, ct_axis=ct_axis, order="block" if k % 2 else "line")
    i0, x0 = costa.mx_dual_items(), costa.mx_items()
    run.call(op, alpha, rounding)
    run.check_one_rank(run.expected(op, alpha, rounding), f"dual {NAMES[tq]} {geom} {op} Ct {ct_ord}")
    assert costa.mx_dual_items() > i0 and costa.mx_items() == x0


def test_transform_mx_dual_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for tq, geom, op, ct_ord in ((E4M3, "g203", "T", "C"), (FP4, "g202", "N", "R"), (E3M2, "custom32q", "T", "R")):
            run = Run(costa, tq, _case(tq, geom, op, ct_ord), c_axis=COLS, ct_axis=ROWS)
            run.call(op, 0.75, stream=s)
            s.synchronize()
            run.check_one_rank(run.expected(op, 0.75), f"dual on a stream {NAMES[tq]} {geom} {op}")


@TYPES
def test_transform_mx_dual_sr(costa, tq):
    geom = {E4M3: "g203", E5M2: "custom32", FP4: "g202", E2M3: "g204", E3M2: "custom32q"}[tq]
    run = Run(costa, tq, _case(tq, geom, "T", "C"), c_axis=COLS, ct_axis=COLS)
    run.call("T", 0.625, seed=SEED)
    exp = run.expected("T", 0.625, seed=SEED)
    run.check_one_rank(exp, f"dual SR {NAMES[tq]} {geom}")
    near = run.expected("T", 0.625)
    assert exp[0][1].tobytes() == near[0][1].tobytes() and exp[1][1].tobytes() == near[1][1].tobytes()
    assert raw(exp[0][0][0]) != raw(near[0][0][0]) and raw(exp[1][0][0]) != raw(near[1][0][0])


@pytest.mark.parametrize("seed", [None, SEED], ids=["plain", "sr"])
@pytest.mark.parametrize("geom", ["g203", "custom32"])
@TYPES
def test_dual_equals_two_separate_calls(costa, tq, geom, seed):
    """all four buffers byte-equal to two transform_mx calls (existing code) into fresh buffers"""
    geom = {("g203", 2): "g202", ("g203", 4): "g204", ("custom32", 4): "custom32q"}.get((geom, GROUP[tq]), geom)
    op = "N" if geom.startswith("custom") else "T"
    run = Run(costa, tq, _case(tq, geom, op, "C"), c_axis=ROWS, ct_axis=ROWS)
    ref = Run(costa, tq, _case(tq, geom, op, "C"), c_axis=ROWS, ct_axis=ROWS)
    comm = costa.Comm.self(0)
    run.call(op, 0.75, seed=seed)
    costa.transform_mx(ref.A[0], ref.C[0], comm, op, 0.75, 0.0, c_scales=ref.SC[0].desc, stochastic_seed=seed)
    costa.transform_mx(ref.A[0], ref.Ct[0], comm, OTHER[op], 0.75, 0.0, c_scales=ref.SCt[0].desc, stochastic_seed=seed)
    for got, want, what in ((run.dc, ref.dc, "C"), (run.dct, ref.dct, "Ct")):
        assert host(got[0]).tobytes() == host(want[0]).tobytes(), what
    assert host(run.SC[0].t).tobytes() == host(ref.SC[0].t).tobytes()
    assert host(run.SCt[0].t).tobytes() == host(ref.SCt[0].t).tobytes()
    assert host(run.dc[0]).tobytes() != raw(run.c[0]) and host(run.dct[0]).tobytes() != raw(run.ct[0])


def test_plan_cache(costa):
    """dual, plain (A, C), dual again: all correct, the third a plan hit; and again after release_caches"""
    tq, op = E4M3, "T"
    run = Run(costa, tq, _case(tq, "g203", op, "C"))
    exp = run.expected(op, 0.75)
    plain = mc.expected_transform_mx(F, tq, op, 0.75, 0.0, run.a_case, run.c_case, 1, run.a, run.c, c_axis=ROWS)
    comm = costa.Comm.self(0)
    for release in (False, True):
        costa.release_caches()
        comm = costa.Comm.self(0)
        run.reset()
        run.call(op, 0.75, comm=comm)
        run.check_one_rank(exp, "dual, first")
        if release:
            costa.release_caches()
            comm = costa.Comm.self(0)
        run.reset()
        ct_before = host(run.dct[0]).tobytes()
        costa.transform_mx(run.A[0], run.C[0], comm, op, 0.75, 0.0, c_scales=run.SC[0].desc)
        run.SC[0].check(plain[1], "plain between the dual calls: c_scales")
        mc.assert_bits(host(run.dc[0]), plain[0][0], tq, "plain between the dual calls")
        assert host(run.dct[0]).tobytes() == ct_before
        run.reset()
        st0 = costa.get_stats()
        run.call(op, 0.75, comm=comm)
        st1 = costa.get_stats()
        run.check_one_rank(exp, "dual, again")
        if not release:
            assert st1["plan_hits"] - st0["plan_hits"] == 1 and st1["plan_misses"] == st0["plan_misses"]


# ------------------------------------------------------------------ several ranks on one GPU
@pytest.mark.parametrize("local_first", [False, True], ids=["local-last", "local-first"])
@pytest.mark.parametrize("tq,geom", [(E4M3, "g192"), (E4M3, "g203pad"), (E4M3, "custom32"), (FP4, "g202"),
                                     (FP4, "custom32"), (E2M3, "g204"), (E2M3, "custom32q")],
                         ids=lambda v: NAMES.get(v, v) if isinstance(v, int) else v)
def test_emulated_ranks_2x2(costa, tq, geom, local_first):
    """each rank's C, Ct and its share of both scale tensors are exact, the bytes of other ranks' blocks
    untouched; the fp32 package moves once (the pack_bytes of ONE transform_mx call)"""
    P, op = 4, "T" if geom.startswith("g2") and not geom.endswith("pad") else "N"
    run = Run(costa, tq, _case(tq, geom, op, "R" if local_first else "C", (2, 2)), P=P, c_axis=COLS, ct_axis=COLS,
              sc_fill=0)
    (e1, s1, _), (e2, s2, _) = run.expected(op, 0.75)
    dc.assert_finite(e1 + e2, tq, geom)
    plans = [costa.plan_export_scaled(run.A[r], run.C[r], r, P, op, 0.75, 0.0) for r in range(P)]
    assert sum(p.send_elems for p in plans) > 0 and sum(int(p.local_scaled.size) for p in plans) > 0
    # the reference volume: one plain call of (A, C)
    ref = Run(costa, tq, _case(tq, geom, op, "C", (2, 2)), P=P, c_axis=COLS, ct_axis=COLS, sc_fill=0)
    one = drive(costa, plans, 4, lambda r, comm: costa.transform_mx(ref.A[r], ref.C[r], comm, op, 0.75, 0.0,
                                                                    c_scales=ref.SC[r].desc))
    i0, x0 = costa.mx_dual_items(), costa.mx_items()
    out = drive(costa, plans, 4, lambda r, comm: run.call(op, 0.75, r=r, comm=comm), local_first=local_first)
    assert out.stats["pack_launches"] > 0 and out.stats["unpack_launches"] > 0
    assert out.stats["pack_bytes"] == one.stats["pack_bytes"] > 0
    assert costa.mx_dual_items() > i0 and costa.mx_items() == x0
    same = sr.family(tq)[4]
    m, n = run.c_case.shape()
    for case, exp, bufs, esc, tensors, name in ((run.c_case, e1, run.dc, s1, run.SC, "C"),
                                                (run.ct_case, e2, run.dct, s2, run.SCt, "Ct")):
        merged, n_own = np.zeros(esc.shape, np.uint8), 0
        for r in range(P):
            same(host(bufs[r]), exp[r], tq, f"{geom} rank {r}: {name}")
            own = mc.owned(case, P, r)
            first = own[:, ::32].T  # axis COLS: the rank owns a block with its first element
            mine = np.where(first, esc, 0).astype(np.uint8)
            tensors[r].check(mine, f"{geom} rank {r}: {name} scales")
            merged = np.maximum(merged, mine)
            n_own += int(first.sum())
        assert n_own == esc.size and merged.tobytes() == esc.tobytes()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_mx_dual_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK on mx_dual_kernel (tests/mx_dual_loopback_child.py)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mx_dual_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_ = out[-1].split()
    assert int(n) == 2 and int(packs) > 0 and int(unpacks) > 0, out[-1]
    assert (int(locals_) == 0) == (mode == "1"), out[-1]


# ------------------------------------------------------------------ refusals
def _refused(costa, run, match, **kw):
    """the call is COSTA_ERR_ARG with `match` and all four device buffers keep their bytes"""
    args = dict(A=run.A[0], C=run.C[0], Ct=run.Ct[0], op="N", c_scales=run.SC[0].desc, ct_scales=run.SCt[0].desc,
                rounding="floor")
    args.update(kw)
    with pytest.raises(costa.CostaError, match=match) as e:
        costa.transform_mx_dual(args["A"], args["C"], args["Ct"], costa.Comm.self(0), args["op"], 1.0,
                                c_scales=args["c_scales"], ct_scales=args["ct_scales"], rounding=args["rounding"])
    assert e.value.code == 1, str(e.value)
    assert host(run.dc[0]).tobytes() == raw(run.c[0]) and host(run.dct[0]).tobytes() == raw(run.ct[0])
    assert host(run.SC[0].t).tobytes() == run.SC[0].full0.tobytes()
    assert host(run.SCt[0].t).tobytes() == run.SCt[0].full0.tobytes()
    return str(e.value)


@pytest.fixture
def refusal_run(costa):
    return Run(costa, E4M3, _case(E4M3, "g192", "N", "C"))


def test_refused_source_type(costa, refusal_run):
    run, lay = refusal_run, sr.family(E4M3)[2]
    a8 = dev(np.zeros(run.a_case.buf_elems(0, 1), np.uint8))
    assert "FP8_E4M3" in _refused(costa, run, "must be COSTA_FLOAT", A=lay(costa, run.a_case, 0, a8.data_ptr(), 1, E4M3))


def test_refused_output_types(costa, refusal_run):
    run, lay = refusal_run, sr.family(E4M3)[2]
    msg = _refused(costa, run, "no dual MX transform", Ct=lay(costa, run.ct_case, 0, run.dct[0].data_ptr(), 1, E5M2))
    assert "FP8_E4M3" in msg and "FP8_E5M2" in msg
    cf = dev(np.zeros(run.c_case.buf_elems(0, 1), np.float32))
    ctf = dev(np.zeros(run.ct_case.buf_elems(0, 1), np.float32))
    _refused(costa, run, "no dual MX transform", C=lay(costa, run.c_case, 0, cf.data_ptr(), 1, F),
             Ct=lay(costa, run.ct_case, 0, ctf.data_ptr(), 1, F))


def test_refused_shape_of_ct(costa, refusal_run):
    run, lay = refusal_run, sr.family(E4M3)[2]
    other = dev(np.zeros(run.c_case.buf_elems(0, 1), np.uint8))
    _refused(costa, run, "dual layouts", Ct=lay(costa, run.c_case, 0, other.data_ptr(), 1, E4M3))


def test_refused_twin_rule(costa, refusal_run):
    from casegen import BC
    run, lay = refusal_run, sr.family(E4M3)[2]
    fine = BC(160, 192, 16, 16)
    buf = dev(np.zeros(fine.buf_elems(0, 1), np.uint8))
    msg = _refused(costa, run, "dual layouts", Ct=lay(costa, fine, 0, buf.data_ptr(), 1, E4M3))
    assert "rows" in msg and "columns" in msg
    assert not host(buf).any()


def test_refused_missing_descriptor(costa, refusal_run):
    _refused(costa, refusal_run, "c_scales is required", c_scales=None)
    _refused(costa, refusal_run, "ct_scales is required", ct_scales=None)


def test_refused_strides(costa, refusal_run):
    run = refusal_run
    _refused(costa, run, "c_scales: the strides", c_scales=costa.MxScales(run.SC[0].t.data_ptr(), ROWS, 1, 1))
    _refused(costa, run, "ct_scales: the strides", ct_scales=costa.MxScales(run.SCt[0].t.data_ptr(), ROWS, 0, 1))


def test_refused_rounding(costa, refusal_run):
    run, comm = refusal_run, costa.Comm.self(0)
    with pytest.raises(costa.CostaError, match="rounding must be") as e:  # (the Python wrapper knows two names only)
        costa._check(costa.lib().costa_hip_transform_mx_dual(
            run.A[0].handle, run.C[0].handle, run.Ct[0].handle, b"N", np.float32(1).tobytes(), run.SC[0].desc,
            run.SCt[0].desc, 7, None, comm.handle))
    assert e.value.code == 1
    assert host(run.dc[0]).tobytes() == raw(run.c[0]) and host(run.dct[0]).tobytes() == raw(run.ct[0])


def test_refused_same_layout_object(costa, refusal_run):
    from casegen import BC
    run = refusal_run
    # (square, so that the shapes agree and the identity check is what refuses)
    sq = BC(96, 96, 32, 32)
    b = [dev(np.zeros(sq.buf_elems(0, 1) * k, np.uint8)) for k in (4, 1)]
    lay = sr.family(E4M3)[2]
    A, C = lay(costa, sq, 0, b[0].data_ptr(), 1, F), lay(costa, sq, 0, b[1].data_ptr(), 1, E4M3)
    d = costa.MxScales(run.SC[0].t.data_ptr() + 32, ROWS, 96, 1)
    for ct in (C,):
        with pytest.raises(costa.CostaError, match="layout of its own") as e:
            costa.transform_mx_dual(A, C, ct, costa.Comm.self(0), "N", 1.0, c_scales=d, ct_scales=d)
        assert e.value.code == 1
    assert not host(b[1]).any() and host(run.SC[0].t).tobytes() == run.SC[0].full0.tobytes()


def test_refused_block_rule(costa):
    run = Run(costa, E4M3, _case(E4M3, "bc203", "N", "C"))
    assert "of C:" in _refused(costa, run, "MX block")
    ok_c = costa.MxScales(run.SC[0].t.data_ptr(), COLS, 1024, 1)  # (never reached: the rule fails first)
    assert "MX block" in _refused(costa, run, "MX block", c_scales=ok_c)


def test_refused_host_memory(costa, refusal_run):
    run, lay = refusal_run, sr.family(E4M3)[2]
    m, n = run.c_case.shape()
    hs = np.full((mc.n_blocks(m), n), 0x5A, np.uint8)
    _refused(costa, run, "device-resident", c_scales=costa.MxScales(hs.ctypes.data, ROWS, n, 1))
    hs2 = np.full((mc.n_blocks(n), m), 0x5A, np.uint8)
    _refused(costa, run, "device-resident", ct_scales=costa.MxScales(hs2.ctypes.data, ROWS, m, 1))
    assert (hs == 0x5A).all() and (hs2 == 0x5A).all()
    hct = np.zeros(run.ct_case.buf_elems(0, 1), np.uint8)
    _refused(costa, run, "device-resident", Ct=lay(costa, run.ct_case, 0, hct.ctypes.data, 1, E4M3))
    ha = run.a[0].copy()
    _refused(costa, run, "device-resident", A=lay(costa, run.a_case, 0, ha.ctypes.data, 1, F))
    assert not hct.any()
    # and the call works afterwards
    run.call("N", 1.0)
    run.check_one_rank(run.expected("N", 1.0), "after the refusals")
