"""amax outputs on the GPU: row / column abs-max vectors updated by the scaled kernels
(costa_hip_transform_amax, costa_hip_execute_tiles_amax) and by the reduce-only pass over a layout
(costa_hip_layout_amax); costa_hip.h, "amax outputs"; costa_amd/csrc/scaled_kernels.hip.

Expected vectors come from amax_common.py (existing helpers only) and are compared as unsigned
integers over their whole length; destination buffers are compared bit for bit with
scaled_common's expected values.  Data are gen() values times an exact power of two per global row
and per global column, so an element reduced into the wrong entry changes the answer.  At kernel
level the vectors are raw addresses into the middle of a larger buffer whose 16 entries before and
after the range hold sentinels, and the initial entries are partly above every datum, partly below.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from amax_common import (absbits, assert_moved, assert_vec, expected_layout_amax, expected_tiles_amax,
                         expected_transform_amax, layout_index, matrix_data, tile_data, utype)
from scaled_common import (BF16, D, E4M3, E5M2, ESIZE, F, F_ROWS, H16, NAMES, NPT, PAIR_IDS, PAIRS, assert_bits,
                           assert_finite, ctype, expected_tiles, expected_transform, gen, geometry, make_layout,
                           scales, widen)
from tri_common import distribute

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR = 0x1
BITCOPY, ALPHA, AXPBY = 0, 2, 3
SCAL = [1, 0, -0.5, 0, -0.5, 2.0]  # slot 0: BITCOPY, slot 1: ALPHA, slot 2: AXPBY
PAD = 16  # sentinel entries on each side of a vector
# pairs that also run the unaligned variants / the other geometries
SOME = [(F, F), (D, D), (F, E4M3), (BF16, BF16)]
FIVE = [(F, F), (D, D), (F, E4M3), (E4M3, F), (BF16, BF16)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def host(t, code):
    return t.cpu().numpy().view(NPT[code])


def vec(v):
    return None if v is None else torch.from_numpy(v.copy()).cuda()


def init_vec(n, ct):
    """entries above every datum (2^20), zero, and below every datum that matters (2^-30), in turn"""
    v = np.zeros(n, ct)
    v[0::3] = 2.0 ** 20
    v[2::3] = 2.0 ** -30
    return v


class RawVec:
    """a vector in the middle of a larger device buffer, PAD sentinel entries on each side"""

    def __init__(self, init):
        self.U, self.ct, self.n = utype(init.dtype), init.dtype, init.size
        full = (self.U(0xDEADBEEF) << self.U(8 * self.U().itemsize - 32)) + np.arange(2 * PAD + self.n).astype(self.U)
        full[PAD:PAD + self.n] = init.view(self.U)
        self.full0 = full.copy()
        self.t = dev(full)
        self.addr = self.t.data_ptr() + PAD * self.U().itemsize

    def read(self, what):
        got = self.t.cpu().numpy().view(self.U)
        for side in (slice(0, PAD), slice(PAD + self.n, None)):
            assert got[side].tobytes() == self.full0[side].tobytes(), f"{what}: a sentinel changed"
        return got[PAD:PAD + self.n].view(self.ct)


# ------------------------------------------------------------------ kernel level
# (source shift, destination shift) in elements; a shifted side also has an odd ld
VARIANTS = {"aligned": (0, 0), "src1": (1, 0), "dst3": (0, 3)}


def _place(at, fast, slow, off):
    ld = (fast + 15) // 16 * 16
    if off:
        return at + off, ld + 1, (at + off + (ld + 1) * slow + 15) // 16 * 16
    return at, ld, at + ld * slow


def _tile_list(costa, sizes, kinds, transpose, variant, coords):
    """every op size x scale kind as ONE list, each op with its own source and destination region
    and (row0, col0) = coords(k); F_ROWS alternates.  Offsets in ELEMENTS.
    -> (ops, source elements, destination elements, rows, columns of the vectors)"""
    s_off, d_off = VARIANTS[variant]
    ops = np.zeros(len(sizes) * len(kinds), costa.SCALED_OP_DTYPE)
    src_at = dst_at = m = n = k = 0
    for nf, ns in sizes:
        for kind, slot in kinds:
            s0, lds, src_at = _place(src_at, nf, ns, s_off)
            df, dslow = (ns, nf) if transpose else (nf, ns)
            d0, ldd, dst_at = _place(dst_at, df, dslow, d_off)
            frow = k % 2 == 0
            row0, col0 = coords(k)
            flags = (TR if transpose else 0) | kind << 4 | slot << 16 | (F_ROWS if frow else 0)
            ops[k] = ((s0, d0, nf, ns, lds, ldd, flags, 0), row0, col0)
            m = max(m, row0 + (nf if frow else ns))
            n = max(n, col0 + (ns if frow else nf))
            k += 1
    return ops, src_at + 16, dst_at + 16, m + 5, n + 5  # (5 entries no op touches)


def _subtiles(costa, ta, tc, ops):
    bf, bs = costa.scaled_subtile(ta, tc)
    return sum(-(-int(o["op"]["nf"]) // bf) * -(-int(o["op"]["ns"]) // bs) for o in ops)


def _run_list(costa, ta, tc, ops, n_src, n_dst, m, n, scale_which, amax_which, what, src=None, finite=True):
    ct = ctype(ta, tc)
    scal = np.array(SCAL, ct)
    if src is None:
        src = tile_data(ta, 0xA1, ops, n_src)
    dst0 = gen(tc, 0xC1, n_dst)
    r = scales(m, 0x11, ct) if "r" in scale_which else None
    cs = scales(n, 0x12, ct) if "c" in scale_which else None
    exp = expected_tiles(costa, ta, tc, ops, scal, src, dst0, r, cs)
    r0 = init_vec(m, ct) if "r" in amax_which else None
    c0 = init_vec(n, ct) if "c" in amax_which else None
    er, ec = expected_tiles_amax(ta, tc, ops, src, r0, c0)
    if finite:
        assert_finite(exp, tc, what)
        for e, i0 in ((er, r0), (ec, c0)):
            if e is not None:
                assert_moved(e, i0, what)
                above = i0 == 2.0 ** 20
                assert above.any() and e[above].tobytes() == i0[above].tobytes()  # nothing is that large
    gpu = ops.copy()
    gpu["op"]["src"] = ops["op"]["src"] * ESIZE[ta]
    gpu["op"]["dst"] = ops["op"]["dst"] * ESIZE[tc]
    ds, dd = dev(src), dev(dst0)
    vr = RawVec(r0) if r0 is not None else None
    vc = RawVec(c0) if c0 is not None else None
    a0, s0 = costa.amax_items(), costa.scaled_items()
    costa.execute_tiles_amax(ta, tc, gpu, scal, ds.data_ptr(), dd.data_ptr(), vec(r), vec(cs),
                             vr.addr if vr else None, vc.addr if vc else None)
    assert_bits(host(dd, tc), exp, tc, what + ": destination")
    if vr:
        assert_vec(vr.read(what + " row_amax"), er, what + ": row_amax")
    if vc:
        assert_vec(vc.read(what + " col_amax"), ec, what + ": col_amax")
    subs = _subtiles(costa, ta, tc, ops)
    assert costa.amax_items() - a0 == subs and costa.scaled_items() - s0 == subs
    assert ds.cpu().numpy().tobytes() == np.ascontiguousarray(src).tobytes()
    return er, ec


def _three_ways(costa, ta, tc, lst, what):
    """both vectors with both scales; row_amax alone without scales; col_amax alone with one scale"""
    _run_list(costa, ta, tc, *lst, "rc", "rc", what)
    _run_list(costa, ta, tc, *lst, "", "r", what + ", r only")
    _run_list(costa, ta, tc, *lst, "r", "c", what + ", c only")


def _coords(k):  # several ops share rows and columns; offsets off the multiples of 4
    return 3 * (k % 4) + 1, 5 * (k % 3) + 2


KERNEL_CASES = [(a, c, "aligned") for a, c in PAIRS] + [(a, c, v) for a, c in SOME for v in ("src1", "dst3")]


@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc,variant", KERNEL_CASES, ids=[f"{NAMES[a]}-{NAMES[c]}-{v}" for a, c, v in KERNEL_CASES])
def test_amax_kernel_tile_lists(costa, ta, tc, variant, transpose):
    bf, bs = costa.scaled_subtile(ta, tc)
    sizes = [(1, 1), (3, 5), (17, 33), (bf + 1, bs + 1), (2 * bf - 1, 7), (7, 2 * bs - 1)]
    kinds = [(BITCOPY, 0), (ALPHA, 1), (AXPBY, 2)]
    lst = _tile_list(costa, sizes, kinds, transpose, variant, _coords)
    assert (lst[0]["row0"] % 4 != 0).any() and (lst[0]["col0"] % 4 != 0).any()
    _three_ways(costa, ta, tc, lst, f"{NAMES[ta]}->{NAMES[tc]} {'T' if transpose else 'N'} {variant}")


@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_amax_kernel_full_path(costa, ta, tc, transpose):
    """whole aligned sub-tiles with target coordinates on multiples of 4: the unguarded path"""
    bf, bs = costa.scaled_subtile(ta, tc)
    lst = _tile_list(costa, [(2 * bf, bs)], [(AXPBY, 2), (ALPHA, 1)], transpose, "aligned",
                     lambda k: (8 + 4 * k, 12 + 8 * k))
    _three_ways(costa, ta, tc, lst, f"{NAMES[ta]}->{NAMES[tc]} {'T' if transpose else 'N'} full")


@pytest.mark.parametrize("wide", [False, True], ids=["bf-x-64bs", "64bf-x-bs"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("code", [F, D], ids=["f32", "f64"])
def test_amax_kernel_contention(costa, code, transpose, wide):
    """64 sub-tiles of one op update the same 64 entries of one vector"""
    bf, bs = costa.scaled_subtile(code, code)
    size = (64 * bf, bs) if wide else (bf, 64 * bs)
    lst = _tile_list(costa, [size], [(ALPHA, 1)], transpose, "aligned", lambda k: (4, 8))
    _run_list(costa, code, code, *lst, "rc", "rc", f"{NAMES[code]} contention")


SPECIAL_BITS = {  # code: (-0, a denormal, +inf, -inf, a NaN); None where the type has none
    F: (0x80000000, 0x00000123, 0x7F800000, 0xFF800000, 0x7FC00001),
    D: (0x8000000000000000, 0x0000000000000123, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001),
    BF16: (0x8000, 0x0023, 0x7F80, 0xFF80, 0x7FC1),
    E4M3: (0x80, 0x03, None, None, 0x7F),
}


@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc", [(F, F), (D, D), (BF16, F), (E4M3, F)], ids=["f32-f32", "f64-f64", "bf16-f32", "e4m3-f32"])
def test_amax_specials(costa, ta, tc, transpose):
    """-0, a denormal, +-inf and a NaN in known rows (the op's fast index walks rows)"""
    nf, ns = 40, 24
    ops = np.zeros(1, costa.SCALED_OP_DTYPE)
    ldd = 32 if transpose else 48
    ops[0] = ((0, 0, nf, ns, 48, ldd, (TR if transpose else 0) | BITCOPY << 4 | F_ROWS, 0), 2, 3)
    m, n = 2 + nf + 4, 3 + ns + 4
    src = tile_data(ta, 0xA7, ops, 48 * ns + 16)
    Us = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[src.dtype.itemsize]
    bits = src.view(Us).copy()
    nz, den, pinf, ninf, nan = SPECIAL_BITS[ta]
    R_ZERO, R_DEN, R_PINF, R_NINF, R_NAN = 3, 5, 6, 8, 9  # source rows f (entries 2 + f)
    bits[R_ZERO::48] = nz         # only -0
    bits[R_DEN::48] = nz          # -0 and one denormal
    bits[R_DEN + 48 * 7] = den
    if pinf is not None:
        bits[R_PINF + 48 * 2] = pinf   # +inf among ordinary values
        bits[R_NINF + 48 * 11] = ninf  # -inf
    bits[R_NAN + 48 * 5] = nan    # a NaN, in column 3 + 5
    src = bits.view(src.dtype)
    ct = ctype(ta, tc)
    # (the run's own expected vectors treat the specials like every other value; then the known rows)
    er, ec = _run_list(costa, ta, tc, ops, 48 * ns + 16, ldd * (nf if transpose else ns) + 16, m, n, "", "rc",
                       f"specials {NAMES[ta]}", src=src, finite=False)
    r0 = init_vec(m, ct)
    Uc = utype(ct)
    e, i0 = er.view(Uc), r0.view(Uc)
    wden = absbits(widen(np.array([den], Us).view(src.dtype), ta).astype(ct))[0]
    inf_bits = absbits(np.array([np.inf], ct))[0]
    assert wden != 0 and not np.isnan(er[2 + R_DEN])
    untouched = [k for k in range(m) if k < 2 or k >= 2 + nf]
    assert er[untouched].tobytes() == r0[untouched].tobytes()
    # (the chosen rows start from an initial entry a datum can raise: 0 or 2^-30, not 2^20)
    assert all(r0[2 + f] < 1 for f in (R_ZERO, R_DEN, R_PINF, R_NINF, R_NAN)) and r0[2 + R_DEN] == 0
    assert e[2 + R_ZERO] == i0[2 + R_ZERO]  # -0 became +0: nothing to raise
    assert e[2 + R_DEN] == wden
    if pinf is not None:
        assert e[2 + R_PINF] == inf_bits and e[2 + R_NINF] == inf_bits
    assert np.isnan(er[2 + R_NAN]) and np.isnan(ec[3 + 5])


# ------------------------------------------------------------------ transform level
def _scalars(op):
    return (1, 0) if op == "N" else (-0.5, 2.0)


def _torch_ct(ct):
    return torch.float64 if np.dtype(ct) == np.float64 else torch.float32


def _xf(costa, ta, tc, geom, op, scale_which="rc", amax_which="rc", launch=None, seeds=(0x51, 0x52), cases=None):
    """one transform_amax on fresh layouts; -> what, got C, expected C, [(got vector, expected, initial)]"""
    a_case, c_case = cases or geometry(geom, op)
    alpha, beta = _scalars(op)
    ct = ctype(ta, tc)
    m, n = c_case.shape()
    a = matrix_data(ta, seeds[0], a_case)
    c = gen(tc, seeds[1], c_case.buf_elems(0, 1))
    r = scales(m, seeds[0] + 7, ct) if "r" in scale_which else None
    cs = scales(n, seeds[1] + 7, ct) if "c" in scale_which else None
    exp = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c, r, cs)
    assert_finite(exp, tc, f"{geom} {op}")
    r0 = np.zeros(m, ct) if "r" in amax_which else None
    c0 = np.zeros(n, ct) if "c" in amax_which else None
    er, ec = expected_transform_amax(ta, tc, op, a_case, c_case, a, r0, c0)
    da, dc, dr, dcs, ra, ca = dev(a), dev(c), vec(r), vec(cs), vec(r0), vec(c0)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    if launch is None:
        costa.transform_amax(A, C, costa.Comm.self(0), op, alpha, beta, dr, dcs, ra, ca)
    else:
        launch(A, C, alpha, beta, dr, dcs, ra, ca)
    vecs = [(g.cpu().numpy(), e, i0) for g, e, i0 in ((ra, er, r0), (ca, ec, c0)) if g is not None]
    return host(dc, tc), exp, vecs


def _check(ta, tc, got, exp, vecs, what):
    assert_bits(got, exp, tc, what + ": C")
    for k, (g, e, i0) in enumerate(vecs):
        assert_moved(e, i0, f"{what}: vector {k}")
        assert_vec(g, e, f"{what}: vector {k}")


XF_CASES = [(a, c, "bc203") for a, c in PAIRS] + [(a, c, g) for g in ("cfg5", "lldpad") for a, c in FIVE]


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("ta,tc,geom", XF_CASES, ids=[f"{NAMES[a]}-{NAMES[c]}-{g}" for a, c, g in XF_CASES])
def test_transform_amax_matches_oracle(costa, ta, tc, geom, op):
    a0 = costa.amax_items()
    got, exp, vecs = _xf(costa, ta, tc, geom, op)
    _check(ta, tc, got, exp, vecs, f"{NAMES[ta]}->{NAMES[tc]} {op} {geom}")
    assert len(vecs) == 2 and costa.amax_items() > a0


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("ta,tc", [(F, F), (F, H16), (E5M2, F)], ids=["f32-f32", "f32-f16", "e5m2-f32"])
def test_transform_amax_without_scales(costa, ta, tc, op):
    """both scales None: the scaled definition with both products skipped, plus the vectors"""
    got, exp, vecs = _xf(costa, ta, tc, "bc203", op, scale_which="")
    _check(ta, tc, got, exp, vecs, f"no scales {NAMES[ta]}->{NAMES[tc]} {op}")
    got, exp, vecs = _xf(costa, ta, tc, "bc203", op, scale_which="", amax_which="c")
    _check(ta, tc, got, exp, vecs, f"no scales, col_amax only {NAMES[ta]}->{NAMES[tc]} {op}")
    assert len(vecs) == 1


def test_transform_amax_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    comm = costa.Comm.self(0)

    def launch(A, C, alpha, beta, dr, dcs, ra, ca):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            costa.transform_amax(A, C, comm, "T", alpha, beta, dr, dcs, ra, ca, stream=s)
        s.synchronize()
    got, exp, vecs = _xf(costa, F, E4M3, "bc203", "T", launch=launch)
    _check(F, E4M3, got, exp, vecs, "async f32->e4m3 T")


@pytest.mark.parametrize("code", [F, D], ids=["f32", "f64"])
def test_transform_amax_in_place(costa, code):
    """A <- diag(r) * A * diag(c) on one handle; the amax is that of the matrix before scaling"""
    _, case = geometry("lldpad", "N")
    ct = ctype(code, code)
    m, n = case.shape()
    a = matrix_data(code, 0x41, case)
    r, cs = scales(m, 0x42, ct), scales(n, 0x43, ct)
    exp = expected_transform(code, code, "N", 1, 0, case, case, a, a.copy(), r, cs)
    assert_finite(exp, code, "in place")
    r0, c0 = np.zeros(m, ct), np.zeros(n, ct)
    er, ec = expected_transform_amax(code, code, "N", case, case, a, r0, c0)
    da, ra, ca = dev(a), vec(r0), vec(c0)
    A = make_layout(costa, case, 0, da.data_ptr(), 1, code)
    costa.transform_amax(A, A, costa.Comm.self(0), "N", 1, 0, vec(r), vec(cs), ra, ca)
    _check(code, code, host(da, code), exp, [(ra.cpu().numpy(), er, r0), (ca.cpu().numpy(), ec, c0)],
           f"in place {NAMES[code]}")
    # the matrix after scaling has another amax (|r| reaches 2): the vectors are not that
    ar, _ = expected_transform_amax(code, code, "N", case, case, exp, r0, c0)
    assert ar.tobytes() != er.tobytes()


def test_transform_amax_accumulates_over_calls(costa):
    """two calls on different A update the same vectors"""
    ta, tc, op = BF16, F, "T"
    a_case, c_case = geometry("bc203", op)
    m, n = c_case.shape()
    a1, a2 = matrix_data(ta, 0x21, a_case), matrix_data(ta, 0x22, a_case)
    c = gen(tc, 0x23, c_case.buf_elems(0, 1))
    r0, c0 = np.zeros(m, np.float32), np.zeros(n, np.float32)
    r1, c1 = expected_transform_amax(ta, tc, op, a_case, c_case, a1, r0, c0)
    r2, c2 = expected_transform_amax(ta, tc, op, a_case, c_case, a2, r1, c1)
    assert r2.tobytes() != r1.tobytes() and c2.tobytes() != c1.tobytes()
    only2, _ = expected_transform_amax(ta, tc, op, a_case, c_case, a2, r0, c0)
    assert r2.tobytes() != only2.tobytes()
    d1, d2, dc, ra, ca = dev(a1), dev(a2), dev(c), vec(r0), vec(c0)
    comm = costa.Comm.self(0)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    for d in (d1, d2):
        costa.transform_amax(make_layout(costa, a_case, 0, d.data_ptr(), 1, ta), C, comm, op, 1, 0,
                             row_amax=ra, col_amax=ca)
    assert_vec(ra.cpu().numpy(), r2, "accumulated row_amax")
    assert_vec(ca.cpu().numpy(), c2, "accumulated col_amax")
    assert_bits(host(dc, tc), expected_transform(ta, tc, op, 1, 0, a_case, c_case, a2, c), tc, "C of the second call")


def test_scaled_amax_and_ordinary_calls_share_handles_and_one_scaled_plan(costa):
    """transform_scaled, transform_amax, transform on the same two handles: each C is right, and the
    amax call reuses the scaled plan (one miss for it, one for the ordinary plan)"""
    from casegen import BC
    ta = tc = F
    op, (alpha, beta) = "T", _scalars("T")
    a_case, c_case = BC(77, 131, 24, 40), BC(131, 77, 16, 56)  # (a geometry no other test plans)
    m, n = c_case.shape()
    a, c = matrix_data(ta, 0x31, a_case), gen(tc, 0x32, c_case.buf_elems(0, 1))
    da, dc = dev(a), dev(c)
    c_dev0 = dc.clone()
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    comm = costa.Comm.self(0)
    r, cs = scales(m, 1, np.float32), scales(n, 2, np.float32)
    exp_s = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c, r, cs)
    exp_0 = c.copy()
    oracle.transform(oracle.FLOAT, op, alpha, beta, a_case.geom(1), [a], c_case.geom(1), [exp_0])
    r0, c0 = np.zeros(m, np.float32), np.zeros(n, np.float32)
    er, ec = expected_transform_amax(ta, tc, op, a_case, c_case, a, r0, c0)
    ra, ca = vec(r0), vec(c0)
    st0 = costa.get_stats()
    costa.transform_scaled(A, C, comm, op, alpha, beta, vec(r), vec(cs))
    st1 = costa.get_stats()
    assert_bits(host(dc, tc), exp_s, tc, "scaled")
    dc.copy_(c_dev0)
    costa.transform_amax(A, C, comm, op, alpha, beta, vec(r), vec(cs), ra, ca)
    st2 = costa.get_stats()
    assert_bits(host(dc, tc), exp_s, tc, "amax")
    assert_vec(ra.cpu().numpy(), er, "row_amax")
    assert_vec(ca.cpu().numpy(), ec, "col_amax")
    dc.copy_(c_dev0)
    costa.transform(A, C, comm, op, alpha, beta)
    st3 = costa.get_stats()
    assert_bits(host(dc, tc), exp_0, tc, "ordinary")
    assert st1["plan_misses"] - st0["plan_misses"] == 1
    assert st2["plan_misses"] == st1["plan_misses"] and st2["plan_hits"] - st1["plan_hits"] == 1
    assert st3["plan_misses"] - st2["plan_misses"] == 1


# ------------------------------------------------------------------ layout_amax
LAYOUT_GEOMS = ["bc203", "cfg5", "lldpad", "rowmajor"]


def _layout_case(geom):
    if geom == "rowmajor":
        from casegen import BC
        return BC(203, 157, 40, 24, pm=2, pn=2, ord="R", lld_pad=1)
    return geometry(geom, "N", grid=(2, 2))[0]


@pytest.mark.parametrize("geom", LAYOUT_GEOMS)
@pytest.mark.parametrize("code", [F, D, H16, BF16, E4M3, E5M2], ids=lambda c: NAMES[c])
def test_layout_amax_per_rank(costa, code, geom):
    """the layouts of ranks 0..3 of 4 on one device: each rank's vectors are the maxima over its own
    elements, their elementwise maximum the whole matrix's; huge values in the padding do not leak"""
    case = _layout_case(geom)
    P = 4
    ct = np.float64 if code == D else np.float32
    m, n = case.shape()
    comm = costa.Comm.self(0)
    huge = {F: 3.0e38, D: 1.0e300, H16: 60000.0, BF16: 3.0e38, E4M3: 448.0, E5M2: 57344.0}[code]
    from scaled_common import cvt
    huge_el = cvt(np.array([huge], ct), code)[0]
    whole_r, whole_c = np.zeros(m, ct), np.zeros(n, ct)
    a0 = costa.amax_items()
    for rank in range(P):
        a = matrix_data(code, 0x90 + rank, case, P, rank)
        pad = ~layout_index(case, P)[rank][2]
        a[pad] = huge_el
        r0, c0 = np.zeros(m, ct), np.zeros(n, ct)
        er, ec = expected_layout_amax(code, case, a, P, rank, r0, c0)
        assert_moved(er, r0, f"rank {rank} rows")
        assert_moved(ec, c0, f"rank {rank} columns")
        assert max(er.max(), ec.max()) < huge
        da, ra, ca = dev(a), vec(r0), vec(c0)
        costa.layout_amax(make_layout(costa, case, rank, da.data_ptr(), P, code), comm, ra, ca)
        assert_vec(ra.cpu().numpy(), er, f"{NAMES[code]} {geom} rank {rank}: row_amax")
        assert_vec(ca.cpu().numpy(), ec, f"{NAMES[code]} {geom} rank {rank}: col_amax")
        assert da.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
        whole_r, whole_c = np.maximum(whole_r, ra.cpu().numpy()), np.maximum(whole_c, ca.cpu().numpy())
        if geom == "lldpad":
            assert pad.any()
    assert costa.amax_items() > a0
    # the dense matrix the four ranks hold: every rank's buffer came from its own seed, so rebuild it
    # from the ranks' expected vectors' inputs through one accumulation over all four
    acc_r, acc_c = np.zeros(m, ct), np.zeros(n, ct)
    for rank in range(P):
        a = matrix_data(code, 0x90 + rank, case, P, rank)
        acc_r, acc_c = expected_layout_amax(code, case, a, P, rank, acc_r, acc_c)
    assert_vec(whole_r, acc_r, "elementwise maximum over the ranks: rows")
    assert_vec(whole_c, acc_c, "elementwise maximum over the ranks: columns")
    assert (acc_r > 0).all() and (acc_c > 0).all()  # the four ranks cover every row and column


def test_layout_amax_one_vector_and_async(costa):
    case = _layout_case("lldpad")
    m, n = case.shape()
    a = matrix_data(F, 0x95, case, 4, 1)
    r0, c0 = np.zeros(m, np.float32), np.zeros(n, np.float32)
    er, ec = expected_layout_amax(F, case, a, 4, 1, r0, c0)
    da, ra, ca = dev(a), vec(r0), vec(c0)
    A = make_layout(costa, case, 1, da.data_ptr(), 4, F)
    comm = costa.Comm.self(0)
    costa.layout_amax(A, comm, row_amax=ra)
    assert_vec(ra.cpu().numpy(), er, "row_amax alone")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        costa.layout_amax(A, comm, col_amax=ca, stream=s)
        twice = ca * 2  # queued on the stream behind the call
    s.synchronize()
    assert_vec(ca.cpu().numpy(), ec, "col_amax alone, stream-ordered")
    assert_vec(twice.cpu().numpy(), ec * 2, "work queued behind the call sees the result")


# ------------------------------------------------------------------ the two recipes
def _quantisation_case():
    """the data of test_gpu_scaled.py::test_per_channel_quantisation_on_torch_tensors"""
    a_case, c_case = geometry("bc203", "N")
    m, n = c_case.shape()
    pw = np.float32(2.0) ** ((np.arange(m) * 7) % 20 - 6).astype(np.float32)
    M = oracle.gen(oracle.FLOAT, 0xB1, 0, m * n).reshape(m, n) * pw[:, None]
    assert M.dtype == np.float32
    a32 = distribute(M, a_case, 1)[0].astype(np.float32)
    amax = np.abs(M).max(axis=1)
    c0 = gen(E4M3, 0xB2, c_case.buf_elems(0, 1))
    return a_case, c_case, m, n, a32, amax, c0


def test_current_scaling_on_the_device(costa):
    """layout_amax on an fp32 torch tensor, 448 / amax in torch, transform_scaled into a
    float8_e4m3fn tensor: bit-equal to the host recipe, and nothing left the device in between"""
    a_case, c_case, m, n, a32, amax, c0 = _quantisation_case()
    row_scale = (np.float32(448) / amax).astype(np.float32)
    exp = expected_transform(F, E4M3, "N", 1, 0, a_case, c_case, a32, c0, r=row_scale)
    assert_finite(exp, E4M3, "quantise")
    ta = torch.from_numpy(a32).cuda()
    tq = torch.from_numpy(c0.copy()).cuda().view(torch.float8_e4m3fn)
    A = make_layout(costa, a_case, 0, ta.data_ptr(), 1, costa.element_code(ta.dtype))
    C = make_layout(costa, c_case, 0, tq.data_ptr(), 1, costa.element_code(tq.dtype))
    comm = costa.Comm.self(0)
    t_amax = torch.zeros(m, dtype=torch.float32, device="cuda")
    costa.layout_amax(A, comm, row_amax=t_amax)
    t_scale = 448 / t_amax
    costa.transform_scaled(A, C, comm, "N", 1, 0, row_scale=t_scale)
    assert_vec(t_amax.cpu().numpy(), amax, "amax")
    assert_bits(tq.view(torch.uint8).cpu().numpy(), exp, E4M3, "current scaling fp32 -> e4m3")


def test_delayed_scaling(costa):
    """transform_amax fp32 -> e4m3 with a given row_scale (the previous step's) and a row_amax output"""
    a_case, c_case, m, n, a32, amax, c0 = _quantisation_case()
    prev_scale = (np.float32(448) / (amax * np.float32(1.5))).astype(np.float32)
    exp = expected_transform(F, E4M3, "N", 1, 0, a_case, c_case, a32, c0, r=prev_scale)
    assert_finite(exp, E4M3, "quantise")
    ta = torch.from_numpy(a32).cuda()
    tq = torch.from_numpy(c0.copy()).cuda().view(torch.float8_e4m3fn)
    A = make_layout(costa, a_case, 0, ta.data_ptr(), 1, F)
    C = make_layout(costa, c_case, 0, tq.data_ptr(), 1, E4M3)
    t_amax = torch.zeros(m, dtype=torch.float32, device="cuda")
    costa.transform_amax(A, C, costa.Comm.self(0), "N", 1, 0, row_scale=torch.from_numpy(prev_scale).cuda(),
                         row_amax=t_amax)
    assert_bits(tq.view(torch.uint8).cpu().numpy(), exp, E4M3, "delayed scaling: C")
    assert_vec(t_amax.cpu().numpy(), amax, "delayed scaling: row_amax")


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_unchanged(costa):
    a_case, c_case = geometry("bc203", "N")
    m, n = c_case.shape()
    comm = costa.Comm.self(0)
    a, c = matrix_data(F, 1, a_case), gen(F, 2, c_case.buf_elems(0, 1))
    r = scales(m, 3, np.float32)
    dr = vec(r)
    r0 = np.zeros(m, np.float32)
    ra = vec(r0)
    # host-resident layouts
    c_host = c.copy()
    A = make_layout(costa, a_case, 0, a.ctypes.data, 1, F)
    C = make_layout(costa, c_case, 0, c_host.ctypes.data, 1, F)
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.transform_amax(A, C, comm, row_scale=dr, row_amax=ra)
    assert e.value.code == 1 and c_host.tobytes() == c.tobytes()
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.layout_amax(A, comm, row_amax=ra)
    assert e.value.code == 1
    da, dc = dev(a), dev(c)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, F)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, F)
    # both amax vectors None; a host address for one
    with pytest.raises(costa.CostaError, match="costa_hip_transform_scaled") as e:
        costa.transform_amax(A, C, comm, row_scale=dr)
    assert e.value.code == 1 and "costa_hip_transform" in str(e.value)
    with pytest.raises(costa.CostaError) as e:
        costa.layout_amax(A, comm)
    assert e.value.code == 1
    h = r0.copy()
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.transform_amax(A, C, comm, row_scale=dr, row_amax=h.ctypes.data)
    assert e.value.code == 1
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.layout_amax(A, comm, row_amax=h.ctypes.data)
    assert e.value.code == 1 and h.tobytes() == r0.tobytes()
    # tensors of the wrong dtype or length
    for bad in (torch.zeros(m + 1, dtype=torch.float32, device="cuda"),
                torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float32)):
        with pytest.raises(ValueError):
            costa.transform_amax(A, C, comm, row_scale=dr, row_amax=bad)
        with pytest.raises(ValueError):
            costa.layout_amax(A, comm, row_amax=bad)
    # complex and int32 layouts
    for code, name in ((costa.CFLOAT, "CFLOAT"), (costa.CDOUBLE, "CDOUBLE"), (costa.INT32, "INT32")):
        buf = torch.zeros(a_case.buf_elems(0, 1) * 16, dtype=torch.uint8, device="cuda")
        L = a_case.make_layout(0, buf.data_ptr(), 1, code)
        with pytest.raises(costa.CostaError) as e:
            costa.layout_amax(L, comm, row_amax=ra)
        assert e.value.code == 1 and name.lower() in str(e.value).lower(), str(e.value)
    # an unsupported pair is refused as for scaled transforms (a raw address: the tensor check would
    # ask for the float64 of a DOUBLE target first)
    db = torch.zeros(c_case.buf_elems(0, 1) * 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(costa.CostaError, match="FLOAT") as e:
        costa.transform_amax(A, make_layout(costa, c_case, 0, db.data_ptr(), 1, D), comm, row_amax=ra.data_ptr())
    assert e.value.code == 1 and "DOUBLE" in str(e.value)
    assert dc.cpu().numpy().tobytes() == c.tobytes() and ra.cpu().numpy().tobytes() == r0.tobytes()
    # and the calls work afterwards
    costa.transform_amax(A, C, comm, row_scale=dr, row_amax=ra)
    assert_bits(host(dc, F), expected_transform(F, F, "N", 1, 0, a_case, c_case, a, c, r), F, "after refusals")
    er, _ = expected_transform_amax(F, F, "N", a_case, c_case, a, r0, None)
    assert_vec(ra.cpu().numpy(), er, "after refusals")
    ra2 = vec(r0)
    costa.layout_amax(A, comm, row_amax=ra2)
    assert_vec(ra2.cpu().numpy(), expected_layout_amax(F, a_case, a, 1, 0, r0, None)[0], "layout_amax after refusals")


# ------------------------------------------------------------------ neighbours
def test_other_transforms_are_unchanged_around_an_amax_call(costa):
    """an ordinary and a scaled transform give identical bytes before and after amax calls, and the
    counters show which instance ran"""
    a_case, c_case = geometry("bc203", "T")
    m, n = c_case.shape()
    comm = costa.Comm.self(0)
    a, c = gen(F, 0x61, a_case.buf_elems(0, 1)), gen(F, 0x62, c_case.buf_elems(0, 1))
    r, cs = scales(m, 0x63, np.float32), scales(n, 0x64, np.float32)

    def run(scaled):
        da, dc = dev(a), dev(c)
        A = make_layout(costa, a_case, 0, da.data_ptr(), 1, F)
        C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, F)
        s0, a0 = costa.scaled_items(), costa.amax_items()
        if scaled:
            costa.transform_scaled(A, C, comm, "T", -0.5, 2.0, vec(r), vec(cs))
            assert costa.scaled_items() > s0
        else:
            costa.transform(A, C, comm, "T", -0.5, 2.0)
            assert costa.scaled_items() == s0
        assert costa.amax_items() == a0  # no amax instance ran
        return dc.cpu().numpy().tobytes()
    before = run(False), run(True)
    s0, a0 = costa.scaled_items(), costa.amax_items()
    got, exp, vecs = _xf(costa, F, F, "bc203", "T")
    _check(F, F, got, exp, vecs, "amax in between")
    ds, da_ = costa.scaled_items() - s0, costa.amax_items() - a0
    assert ds == da_ > 0  # every sub-tile of the call ran on the amax instance
    ra = torch.zeros(a_case.shape()[0], dtype=torch.float32, device="cuda")
    dbuf = dev(a)
    s1, a1 = costa.scaled_items(), costa.amax_items()
    costa.layout_amax(make_layout(costa, a_case, 0, dbuf.data_ptr(), 1, F), comm, row_amax=ra)
    assert costa.scaled_items() == s1 and costa.amax_items() > a1  # the reduce-only kernel
    after = run(False), run(True)
    exp_f = c.copy()
    oracle.transform(oracle.FLOAT, "T", -0.5, 2.0, a_case.geom(1), [a], c_case.geom(1), [exp_f])
    assert before == after
    assert before[0] == exp_f.tobytes()
    assert before[1] == expected_transform(F, F, "T", -0.5, 2.0, a_case, c_case, a, c, r, cs).tobytes()


# ------------------------------------------------------------------ exchange path
@pytest.mark.parametrize("mode", ["1", "2"])
def test_amax_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK on the amax instance (tests/amax_loopback_child.py;
    the mode is fixed per process)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "amax_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_ = out[-1].split()
    assert int(n) == 5 and int(packs) > 0 and int(unpacks) > 0, out[-1]
    if mode == "1":
        assert int(locals_) == 0, out[-1]
    else:
        assert int(locals_) > 0, out[-1]
