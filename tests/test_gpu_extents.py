"""GPU: buffers past 4 GiB and 2^31 elements in every kernel family.

Every kernel computes its sub-tile addresses as int64(s0) * ld + f0 on op records the planners and the
work-list builders made with 64-bit arithmetic of their own.  These tests run the families' ordinary
small cases inside buffers whose leading dimension (or block placement) puts the last quarter of the
local matrix past 2^32 bytes or 2^31 elements from the op's first element (stretch_common.py): the
expected result is the family's CPU reference on the small twin, the touched rectangle is compared
bit for bit, and EVERY other byte of the multi-GiB buffers must still hold the sentinel afterwards.
Before a launch the op lists are checked on the host: every footprint inside its allocation (or
nothing is launched) and the threshold really crossed by the sub-tiles that will run.

Then one op of more than 2^31 elements (46400 x 46400 e4m3) and matrices of 2^22 x 1 / 1 x 2^22 /
3 x 2^21 through the ordinary transform.

Each case prints one line `extents <id> | variants | largest offset | device GiB`; the table of
profiles/extents/README.md is made of them.
"""
import numpy as np
import pytest

import bs_common
import fp4_common
import fp6_common
import fp8_common
import half_common
import mx_common
import oracle
import scaled_common
import stretch_common as sc
from amax_common import assert_vec, expected_transform_amax
from casegen import BC
from tri_common import distribute, keep_mask

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _gpu(costa):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    yield
    costa.set_planner(1)
    costa.set_list_builder(1)
    torch.cuda.empty_cache()


def _ids(specs):
    return [pytest.param(s, id=s.id) for s in specs]


# ------------------------------------------------------------------ inputs and references on the twin
_MX = {"mx": mx_common, "mx4": fp4_common, "mx6": fp6_common, "bs": bs_common}
F, ROWS, COLS = 0, 0, 1


def _mx_inputs(s, na, nc):
    """as the families' own one-rank tests draw them: fp32 data spread over several binades, random
    codes of a narrow type; the scale tensors of aux are compact"""
    if s.ta == F:
        a = mx_common.quant_data(0x31, na)
    else:
        a = {"mx": lambda: mx_common.cvt(mx_common.quant_data(0x32, na), s.ta), "mx4": lambda: fp4_common.fp4_data(0x32, na),
             "mx6": lambda: fp6_common.fp6_data(0x32, na), "bs": lambda: bs_common.cvt(bs_common.quant_data(0x32, na), s.ta)}[s.family]()
    c = {"mx": lambda: fp8_common.gen(s.tc, 0x33, nc), "mx4": lambda: fp4_common.fill(s.tc, 0x33, nc),
         "mx6": lambda: fp6_common.fill(s.tc, 0x33, nc), "bs": lambda: fp8_common.gen(s.tc, 0x33, nc)}[s.family]()
    return a, c


def _mx_aux(costa, s):
    """axes / block shapes of the case and its compact scale tensors on the device"""
    kind, t = s.extra["kind"], s.op != "N"
    aux = {}
    if s.family == "bs":
        aux["a_block"], aux["c_block"] = ((128, 128), (1, 128)) if t else ((1, 128), (128, 128))

        def shape(case, block):
            r, c = case.shape()
            return -(-r // block[0]), -(-c // block[1])
        if s.ta != F:
            aux["sa"] = bs_common.scale_floats(0x34, shape(s.a_twin, aux["a_block"]))
            aux["dsa"] = torch.from_numpy(aux["sa"]).cuda()
            aux["a_desc"] = costa.block_scales(aux["dsa"], aux["a_block"], s.a_twin.shape())
        if s.tc != F:
            aux["dsc"] = torch.zeros(shape(s.c_twin, aux["c_block"]), dtype=torch.float32, device="cuda")
            aux["c_desc"] = costa.block_scales(aux["dsc"], aux["c_block"], s.c_twin.shape())
        return aux
    # (requantise 'T' turns the block axis round, 'N' keeps it)
    aux["a_axis"] = COLS if t else ROWS
    aux["c_axis"] = (ROWS if aux["a_axis"] == COLS else COLS) if kind == "requantise" and t else aux["a_axis"]

    def shape(case, axis):
        r, c = case.shape()
        return ((r + 31) // 32, c) if axis == ROWS else ((c + 31) // 32, r)
    if s.ta != F:
        aux["sa"] = mx_common.scale_bytes(0x34, shape(s.a_twin, aux["a_axis"]))
        aux["dsa"] = torch.from_numpy(aux["sa"]).cuda()
        aux["a_desc"] = costa.mx_scales(aux["dsa"], aux["a_axis"], s.a_twin.shape())
    if s.tc != F:
        aux["dsc"] = torch.zeros(shape(s.c_twin, aux["c_axis"]), dtype=torch.uint8, device="cuda")
        aux["c_desc"] = costa.mx_scales(aux["dsc"], aux["c_axis"], s.c_twin.shape())
    return aux


def _mx_expected(s, a, c, aux):
    quant = s.tc != F
    if s.family == "bs":
        exp, esc, _ = bs_common.expected_transform_bs(s.ta, s.tc, s.op, s.alpha, s.beta, s.a_twin, s.c_twin, 1, [a], [c],
                                                      sa=aux.get("sa"), a_block=aux["a_block"],
                                                      c_block=aux["c_block"] if quant else None)
    else:
        fn = {"mx": mx_common.expected_transform_mx, "mx4": fp4_common.expected_transform_mx4,
              "mx6": fp6_common.expected_transform_mx6}[s.family]
        exp, esc, _ = fn(s.ta, s.tc, s.op, s.alpha, s.beta, s.a_twin, s.c_twin, 1, [a], [c], sa=aux.get("sa"),
                         a_axis=aux["a_axis"], c_axis=aux["c_axis"] if quant else None)
    aux["esc"] = esc
    return exp[0]


def _mx_after(s, aux):
    """the compact scale tensors: c_scales exactly the model's, a_scales unchanged"""
    if "dsc" in aux:
        got = aux["dsc"].cpu().numpy()
        if s.family == "bs":
            bs_common.assert_float_bits(got, aux["esc"], s.id + " c_scales")
        else:
            assert got.shape == aux["esc"].shape and np.array_equal(got, aux["esc"]), s.id + " c_scales"
    if "dsa" in aux:
        assert aux["dsa"].cpu().numpy().tobytes() == aux["sa"].tobytes(), s.id + " a_scales were written"


def _inputs(s):
    na, nc = s.a_twin.buf_elems(0, 1), s.c_twin.buf_elems(0, 1)
    if s.family in _MX:
        return _mx_inputs(s, na, nc)
    if s.family in ("plain", "custom", "mixed", "tri"):
        return oracle.gen(s.ta, 0x51, 0, na), oracle.gen(s.tc, 0x52, 0, nc)
    return scaled_common.gen(s.ta, 0x51, na), scaled_common.gen(s.tc, 0x52, nc)


def _expected(s, a, c, aux):
    """the expected twin C buffer from the family's CPU reference"""
    ga, gc = s.a_twin.geom(1), s.c_twin.geom(1)
    if s.family in ("plain", "custom"):
        exp = c.copy()
        oracle.transform(s.tc, s.op, s.alpha, s.beta, ga, [a], gc, [exp])
        return exp
    if s.family == "mixed":
        exp = c.copy()
        with np.errstate(over="ignore", invalid="ignore"):
            oracle.transform(s.tc, s.op, s.alpha, s.beta, ga, [a.astype(oracle.NP[s.tc])], gc, [exp])
        return exp
    if s.family == "half":
        return half_common.expected_transform(s.ta, s.tc, s.op, s.alpha, s.beta, s.a_twin, s.c_twin, a, c)
    if s.family == "fp8":
        return fp8_common.expected_transform(s.ta, s.tc, s.op, s.alpha, s.beta, s.a_twin, s.c_twin, a, c)
    if s.family in ("scaled", "amax"):
        return scaled_common.expected_transform(s.ta, s.tc, s.op, s.alpha, s.beta, s.a_twin, s.c_twin, a, c,
                                                aux.get("r"), aux.get("cs"))
    if s.family in _MX:
        return _mx_expected(s, a, c, aux)
    if s.family == "tri":
        full = c.copy()
        oracle.transform(s.tc, s.op, s.alpha, s.beta, ga, [a], gc, [full])
        m, n = s.c_twin.shape()
        kc = distribute(keep_mask(m, n, s.extra["uplo"], s.extra["k"]).astype(np.float64), s.c_twin, 1)[0]
        assert 0 < kc.sum() < m * n
        return np.where(kc == 1, full, c)
    raise KeyError(s.family)


def _compare(s):
    """the family's own assertion on host arrays (an expected NaN only asks for a NaN)"""
    def cmp(got, exp):
        if s.family in ("half", "fp8", "scaled", "amax"):
            scaled_common.assert_bits(got, exp, s.tc, s.id)
        elif s.family in ("mx", "bs"):
            fp8_common.assert_bits(got, exp, s.tc, s.id)
        elif s.family in ("mx4", "mx6"):
            _MX[s.family].assert_same(got, exp, s.tc, s.id)
        else:
            assert got.tobytes() == exp.tobytes(), f"{s.id}: the touched rectangle differs from the oracle"
    return cmp


def _launch(costa, s, LA, LC, aux):
    comm = costa.Comm.self(0)
    if s.family in ("plain", "custom", "mixed", "half", "fp8"):
        costa.transform(LA, LC, comm, s.op, s.alpha, s.beta)
    elif s.family == "scaled":
        costa.transform_scaled(LA, LC, comm, s.op, s.alpha, s.beta, aux["dr"], aux["dcs"])
    elif s.family == "amax":
        costa.transform_amax(LA, LC, comm, s.op, s.alpha, s.beta, None, None, aux["dra"], aux["dca"])
    elif s.family in ("mx", "mx4", "mx6"):
        costa.transform_mx(LA, LC, comm, s.op, s.alpha, s.beta, a_scales=aux.get("a_desc"), c_scales=aux.get("c_desc"))
    elif s.family == "bs":
        costa.transform_block_scaled(LA, LC, comm, s.op, s.alpha, s.beta, a_scales=aux.get("a_desc"),
                                     c_scales=aux.get("c_desc"))
    elif s.family == "tri":
        costa.transform_tri(LA, LC, comm, s.op, s.extra["uplo"], s.extra["k"], s.alpha, s.beta)
    else:
        raise KeyError(s.family)
    torch.cuda.synchronize()


def _run(costa, s):
    a_big, c_big = s.big()
    total = sc.size_bytes(a_big, s.ta) + sc.size_bytes(c_big, s.tc)
    sc.need(total + (sc.GIB >> 1))
    torch.cuda.reset_peak_memory_stats()
    a, c = _inputs(s)
    aux = _mx_aux(costa, s) if s.family in _MX else {}
    m, n = s.c_twin.shape()
    ct = scaled_common.ctype(s.ta, s.tc) if s.family in ("scaled", "amax") else None
    if s.family == "scaled":  # compact scale vectors
        aux["r"], aux["cs"] = scaled_common.scales(m, 0x71, ct), scaled_common.scales(n, 0x72, ct)
        aux["dr"], aux["dcs"] = torch.from_numpy(aux["r"]).cuda(), torch.from_numpy(aux["cs"]).cuda()
    if s.family == "amax":
        aux["dra"], aux["dca"] = torch.zeros(m, dtype=torch.float32).cuda(), torch.zeros(n, dtype=torch.float32).cuda()
    exp = _expected(s, a, c, aux)
    da = sc.upload(a, s.a_twin, a_big, s.ta)
    dc = sc.upload(c, s.c_twin, c_big, s.tc)
    try:
        if s.family == "plain":
            costa.set_planner(s.mode)
        if s.family == "custom":
            costa.set_list_builder(s.mode)
        costa.release_caches()
        # host checks first: nothing is launched when an op leaves its allocation
        (LA, LC), text, far, plan = sc.host_checks(costa, s, a_big, c_big, da.data_ptr(), dc.data_ptr())
        if s.family == "plain" and s.mode == 2:  # the GPU planner's export: byte-equal to the host's
            d = costa.plan_export([LA], [LC], 0, 1, [s.op], [s.alpha], [s.beta], device=0)
            assert d.local_ops.tobytes() == plan.local_ops.tobytes() and d.scalars.tobytes() == plan.scalars.tobytes()
            assert d.pack_ops.size == 0 and d.unpack_ops.size == 0
        if s.family == "custom" and s.mode == 2:  # ... and the GPU list builder's lists
            h = costa.work_export(s.ta, plan.local_ops)
            g = costa.work_export(s.ta, plan.local_ops, device=0)
            assert g.on_gpu and g.ordered.tobytes() == h.ordered.tobytes() and g.work.tobytes() == h.work.tobytes()
        _launch(costa, s, LA, LC, aux)
        sc.check(dc, exp, s.c_twin, c_big, s.tc, s.id + " C", _compare(s))
        sc.check(da, a, s.a_twin, a_big, s.ta, s.id + " A")
        if s.family in _MX:
            _mx_after(s, aux)
        if s.family == "amax":
            z = np.zeros(m, ct), np.zeros(n, ct)
            er, ec = expected_transform_amax(s.ta, s.tc, s.op, s.a_twin, s.c_twin, a, z[0], z[1])
            assert_vec(aux["dra"].cpu().numpy(), er, s.id + " row amax")
            assert_vec(aux["dca"].cpu().numpy(), ec, s.id + " column amax")
            assert er.max() > 0 and ec.max() > 0
        peak = torch.cuda.max_memory_allocated()
        assert peak <= sc.TEST_LIMIT, f"{peak / sc.GIB:.1f} GiB held"
        print(f"extents {s.id} | {text} | " + ", ".join(f"{k} {v}" for k, v in far.items()) + f" | {peak / sc.GIB:.2f} GiB")
    finally:
        del da, dc
        torch.cuda.empty_cache()


@pytest.mark.parametrize("s", _ids(sc.plain_specs()))
def test_plain_transform_stretched(costa, s):
    _run(costa, s)


@pytest.mark.parametrize("s", _ids(sc.custom_specs()))
def test_two_arena_custom_pair(costa, s):
    _run(costa, s)


@pytest.mark.parametrize("s", _ids(sc.strip_specs()))
def test_strip_family_stretched(costa, s):
    _run(costa, s)


@pytest.mark.parametrize("s", _ids(sc.mx_specs()))
def test_mx_and_block_scaled_stretched(costa, s):
    _run(costa, s)


# ------------------------------------------------------------------ the checker itself
def test_check_finds_a_stray_byte_and_a_wrong_rectangle(costa):
    """stretch_common.check on a small stretched buffer (16 MiB): clean it passes; one byte changed far
    from the rectangle, in a padding row or inside the rectangle fails"""
    twin = BC(40, 30, 40, 30, lld_pad=2)
    big = sc.stretched(twin, 1 << 20)
    a = oracle.gen(oracle.DOUBLE, 3, 0, twin.buf_elems(0, 1))

    def attempt(at):
        t = sc.upload(a, twin, big, 1)
        if at is not None:
            t[at] ^= 1
        sc.check(t, a, twin, big, 1, "self-test")
    attempt(None)
    pitch = 8 * big.sizes(1)[0]
    for at in (5 * pitch + 8 * 42 + 3,          # just below a column's 42 twin rows: the stretched padding
               17 * pitch + pitch // 2,         # far from everything
               sc.big_bytes(big, 1) - 1,        # the last byte
               3 * pitch + 8 * 41,              # the twin's own padding row
               7 * pitch + 8 * 11 + 2):         # an element of the matrix
        with pytest.raises(AssertionError):
            attempt(at)


# ------------------------------------------------------------------ one op of more than 2^31 elements
@pytest.mark.parametrize("op", ["N", "T"])
def test_one_op_past_2_31_elements(costa, op):
    """e4m3 -> e4m3, 46400 x 46400 in one block: 2.15e9 elements in one op, 2.2 GB a side.  Filled
    and checked on the device: C = A or its transpose, the 16 padding rows of every column and the
    tail of both buffers untouched."""
    n, pad, E4M3 = 46400, 16, 7
    case = BC(n, n, n, n, lld_pad=pad)
    lld, total = case.sizes(1)
    assert n * n > 2 ** 31 and total < 2.2e9
    sc.need(5 * total)
    torch.cuda.reset_peak_memory_stats()
    g = torch.Generator(device="cuda").manual_seed(7)
    da = torch.randint(0, 0x7F, (total,), dtype=torch.uint8, device="cuda", generator=g)  # no NaN pattern
    da ^= torch.randint(0, 2, (total,), dtype=torch.uint8, device="cuda", generator=g) << 7
    A = da.view(n, lld)
    A[:, n:] = sc.SENTINEL
    dc = torch.full((total,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
    try:
        LA, LC = case.make_layout(0, da.data_ptr(), 1, E4M3), case.make_layout(0, dc.data_ptr(), 1, E4M3)
        p = costa.plan_export([LA], [LC], 0, 1, [op], [1.0], [0.0])
        assert p.local_ops.size == 1 and int(p.local_ops["nf"][0]) * int(p.local_ops["ns"][0]) > 2 ** 31
        sc.check_footprints(p.local_ops, E4M3, E4M3, (da.data_ptr(), da.data_ptr() + total),
                            (dc.data_ptr(), dc.data_ptr() + total), f"one op {op}")
        keep = da.clone()
        costa.transform(LA, LC, costa.Comm.self(0), op, 1.0, 0.0)
        torch.cuda.synchronize()
        C = dc.view(n, lld)
        want = A[:, :n] if op == "N" else A[:, :n].t()
        assert torch.equal(C[:, :n], want), f"one op of 2^31 elements, {op}"
        assert bool((C[:, n:] == sc.SENTINEL).all()), "padding rows of C written"
        assert torch.equal(da, keep), "the source was written"
        print(f"extents one-op-e4m3-{op} | convert | elements {n * n} | {torch.cuda.max_memory_allocated() / sc.GIB:.2f} GiB")
    finally:
        del da, dc
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ long thin matrices
_THIN = [(1, 1 << 22), (1 << 22, 1), (3, 1 << 21)]


class ThinBC(BC):
    """a one-rank BC whose oracle geometry is written out here: oracle.bc_table returns its block
    counts as nbr * 65536 + nbc, which 65536 blocks along one side overflow"""

    def geom(self, P):
        assert P == 1 and self.pm == self.pn == 1 and self.ia == self.ja == 1 and self.ord == "C"
        lld = self.sizes(1)[0]
        rs = np.append(np.arange(0, self.m, self.mb), self.m).astype(np.int32)
        cs = np.append(np.arange(0, self.n, self.nb), self.n).astype(np.int32)
        tab = np.zeros((rs.size - 1, cs.size - 1, 3), np.int64)
        tab[:, :, 1] = cs[None, :-1].astype(np.int64) * lld + rs[:-1, None]
        tab[:, :, 2] = lld
        return rs, cs, tab.reshape(-1), True


def test_thin_geometry_is_bc_table():
    """... and equals oracle.bc_table where that can say it"""
    for m, n, mb, nb, pad in ((3, 4096, 3, 64, 1), (4096, 1, 64, 1, 0), (1, 1000, 1, 64, 2)):
        a, b = ThinBC(m, n, mb, nb, lld_pad=pad).geom(1), BC(m, n, mb, nb, lld_pad=pad).geom(1)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("code", [1, 7], ids=["f64", "e4m3"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("shape", _THIN, ids=["1x4M", "4Mx1", "3x2M"])
def test_long_thin_matrices(costa, shape, op, code):
    """blocks of 64 along the long side (65536 / 32768 blocks), the whole matrix against the oracle"""
    m, n = shape

    def blk(r, c):
        return min(r, 64), min(c, 64)
    am, an = (n, m) if op == "T" else (m, n)
    a_case, c_case = ThinBC(am, an, *blk(am, an)), ThinBC(m, n, *blk(m, n), lld_pad=1)
    alpha, beta = (1, 0) if op == "N" else (-0.5, 2.0)
    if code == 1:
        a = oracle.gen(code, 0x61, 0, a_case.buf_elems(0, 1))
        c = oracle.gen(code, 0x62, 0, c_case.buf_elems(0, 1))
        exp = c.copy()
        oracle.transform(code, op, alpha, beta, a_case.geom(1), [a], c_case.geom(1), [exp])
    else:
        a = fp8_common.gen(code, 0x61, a_case.buf_elems(0, 1))
        c = fp8_common.gen(code, 0x62, c_case.buf_elems(0, 1))
        exp = fp8_common.expected_transform(code, code, op, alpha, beta, a_case, c_case, a, c)
    da, dc = sc._dev_bytes(a), sc._dev_bytes(c)
    LA = a_case.make_layout(0, da.data_ptr(), 1, code)
    LC = c_case.make_layout(0, dc.data_ptr(), 1, code)
    costa.transform(LA, LC, costa.Comm.self(0), op, alpha, beta)
    got = dc.cpu().numpy().view(exp.dtype)
    if code == 1:
        assert got.tobytes() == exp.tobytes(), f"{m} x {n} {op} f64"
    else:
        fp8_common.assert_bits(got, exp, code, f"{m} x {n} {op} e4m3")
    assert torch.equal(da, sc._dev_bytes(a)), "the source was written"
