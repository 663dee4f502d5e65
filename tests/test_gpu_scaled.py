"""Scaled transforms on the GPU: C(i, j) = beta*C(i, j) + alpha * ((op(A)(i, j) * r[i]) * c[j]) with the
row / column scale vectors fused into the tile kernels (costa_amd/csrc/scaled_kernels.hip; costa_hip.h,
"scaled transforms"), for the 14 accepted pairs.

The expected value is, in every case, the untouched CPU oracle run in the compute type on widened
inputs, with the two products done in numpy and cvt applied once (scaled_common.py).  Results are
compared as raw bits over the WHOLE destination buffer; an expected NaN would only ask for a NaN, so
every generic test also asserts that its expected buffer holds no NaN and no inf (data |x| <= 1,
scales in [0.5, 2), alpha, beta = 1, 0 or -0.5, 2: |result| <= 4 in every type).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from scaled_common import (BF16, D, E4M3, ESIZE, F, F_ROWS, NAMES, NPT, PAIR_IDS, PAIRS, assert_bits,
                           assert_finite, ctype, expected_tiles, expected_transform, gen, geometry, make_layout,
                           scales, widen)
from tri_common import distribute

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR = 0x1
BITCOPY, ALPHA, AXPBY = 0, 2, 3


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


# ------------------------------------------------------------------ kernel level
# (source shift, destination shift) in elements; a shifted side also has an odd ld
VARIANTS = {"aligned": (0, 0), "src1": (1, 0), "dst1": (0, 1), "dst3": (0, 3)}
SCAL = [1, 0, -0.5, 0, -0.5, 2.0]  # slot 0: BITCOPY, slot 1: ALPHA, slot 2: AXPBY


def _place(at, fast, slow, off):
    """region of a fast x slow tile: (first element, ld, next region); regions start on a multiple
    of 16 elements and an unshifted tile has an ld of a multiple of 16; `off` != 0: the tile starts
    that many elements later and its ld is odd"""
    ld = (fast + 15) // 16 * 16
    if off:
        return at + off, ld + 1, (at + off + (ld + 1) * slow + 15) // 16 * 16
    return at, ld, at + ld * slow


def _tile_list(costa, sizes, kinds, transpose, variant, coords):
    """Every op size x scale kind as ONE list: each op has its own region of the source and of the
    destination buffer and its own (row0, col0) = coords(k); F_ROWS alternates.  Offsets in ELEMENTS.
    -> (ops, source elements, destination elements, rows, columns the vectors need)"""
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
    return ops, src_at + 16, dst_at + 16, m, n


def _run_list(costa, ta, tc, ops, n_src, n_dst, m, n, which, what):
    ct = ctype(ta, tc)
    scal = np.array(SCAL, ct)
    src, dst0 = gen(ta, 0xA1, n_src), gen(tc, 0xC1, n_dst)
    r = scales(m, 0x11, ct) if "r" in which else None
    cs = scales(n, 0x12, ct) if "c" in which else None
    exp = expected_tiles(costa, ta, tc, ops, scal, src, dst0, r, cs)
    assert_finite(exp, tc, what)
    gpu = ops.copy()
    gpu["op"]["src"] = ops["op"]["src"] * ESIZE[ta]
    gpu["op"]["dst"] = ops["op"]["dst"] * ESIZE[tc]
    ds, dd, dr, dcs = dev(src), dev(dst0), vec(r), vec(cs)
    items0 = costa.scaled_items()
    costa.execute_tiles_scaled(ta, tc, gpu, scal, ds.data_ptr(), dd.data_ptr(), dr, dcs)
    assert_bits(host(dd, tc), exp, tc, what)
    bf, bs = costa.scaled_subtile(ta, tc)
    subs = sum(-(-int(o["op"]["nf"]) // bf) * -(-int(o["op"]["ns"]) // bs) for o in ops)
    assert costa.scaled_items() - items0 == subs
    assert dst0.tobytes() != exp.tobytes()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_scaled_kernel_tile_lists(costa, ta, tc, transpose, variant):
    bf, bs = costa.scaled_subtile(ta, tc)
    sizes = [(1, 1), (3, 5), (17, 33), (bf + 1, bs + 1), (2 * bf - 1, 7), (7, 2 * bs - 1)]
    kinds = [(BITCOPY, 0), (ALPHA, 1), (AXPBY, 2)]

    def coords(k):  # off every multiple of 4
        return 4 * k + 1 + k % 3, 4 * (k + 2) + 3 - k % 3
    lst = _tile_list(costa, sizes, kinds, transpose, variant, coords)
    assert not ((lst[0]["row0"] % 4 == 0) | (lst[0]["col0"] % 4 == 0)).any()
    what = f"{NAMES[ta]}->{NAMES[tc]} {'T' if transpose else 'N'} {variant}"
    _run_list(costa, ta, tc, *lst, "rc", what)
    if variant == "aligned":
        _run_list(costa, ta, tc, *lst, "r", what + " r only")
        _run_list(costa, ta, tc, *lst, "c", what + " c only")


@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_scaled_kernel_full_path(costa, ta, tc, transpose):
    """one whole aligned sub-tile plus a neighbour, with both senses of F_ROWS and target coordinates
    on multiples of 4: the unguarded path and the vector loads of the scale strips run"""
    bf, bs = costa.scaled_subtile(ta, tc)
    lst = _tile_list(costa, [(2 * bf, bs)], [(AXPBY, 2), (ALPHA, 1)], transpose, "aligned",
                     lambda k: (8 + 4 * k, 12 + 8 * k))
    _run_list(costa, ta, tc, *lst, "rc", f"{NAMES[ta]}->{NAMES[tc]} {'T' if transpose else 'N'} full")


# ------------------------------------------------------------------ transform level
def _scalars(op):
    return (1, 0) if op == "N" else (-0.5, 2.0)


def _run(costa, ta, tc, geom, op, which="rc", launch=None, seeds=(0x51, 0x52), cases=None):
    a_case, c_case = cases or geometry(geom, op)
    alpha, beta = _scalars(op)
    ct = ctype(ta, tc)
    m, n = c_case.shape()
    a = gen(ta, seeds[0], a_case.buf_elems(0, 1))
    c = gen(tc, seeds[1], c_case.buf_elems(0, 1))
    r = scales(m, seeds[0] + 7, ct) if "r" in which else None
    cs = scales(n, seeds[1] + 7, ct) if "c" in which else None
    exp = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c, r, cs)
    assert_finite(exp, tc, f"{geom} {op}")
    da, dc, dr, dcs = dev(a), dev(c), vec(r), vec(cs)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    if launch is None:
        costa.transform_scaled(A, C, costa.Comm.self(0), op, alpha, beta, dr, dcs)
    else:
        launch(A, C, alpha, beta, dr, dcs)
    return host(dc, tc), exp


@pytest.mark.parametrize("geom", ["bc203", "oneblock", "cfg5", "lldpad"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_scaled_transform_matches_oracle(costa, ta, tc, op, geom):
    items0 = costa.scaled_items()
    got, exp = _run(costa, ta, tc, geom, op)
    assert_bits(got, exp, tc, f"{NAMES[ta]}->{NAMES[tc]} {op} {geom}")
    assert costa.scaled_items() > items0


@pytest.mark.parametrize("which", ["r", "c"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_scaled_transform_with_one_vector(costa, ta, tc, op, which):
    got, exp = _run(costa, ta, tc, "whole", op, which)
    assert_bits(got, exp, tc, f"{NAMES[ta]}->{NAMES[tc]} {op} whole, {which} only")


def test_scaled_transform_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    comm = costa.Comm.self(0)

    def launch(A, C, alpha, beta, dr, dcs):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            costa.transform_scaled(A, C, comm, "T", alpha, beta, dr, dcs, stream=s)
        s.synchronize()
    got, exp = _run(costa, F, E4M3, "bc203", "T", launch=launch)
    assert_bits(got, exp, E4M3, "async f32->e4m3 T")


def test_scaled_transform_with_the_gpu_planner_selected(costa):
    """planner mode 2: the GPU planner declines scaled jobs, the host plans, the result is right"""
    from casegen import BC
    costa.set_planner(2)
    try:
        n0 = costa.get_stats()["device_plans"]
        got, exp = _run(costa, F, E4M3, None, "T", cases=(BC(256, 256, 4, 4), BC(256, 256, 8, 8)))
        assert costa.get_stats()["device_plans"] == n0
    finally:
        costa.set_planner(1)
    assert_bits(got, exp, E4M3, "planner mode 2")


def test_plan_cache_keeps_scaled_and_ordinary_plans_apart(costa):
    """on the same two layout handles: scaled, ordinary, scaled with other vector values -- a shared
    cache entry or vectors baked into the plan would show"""
    ta = tc = F
    op, (alpha, beta) = "T", _scalars("T")
    a_case, c_case = geometry("bc203", op)
    m, n = c_case.shape()
    a, c = gen(ta, 0x31, a_case.buf_elems(0, 1)), gen(tc, 0x32, c_case.buf_elems(0, 1))
    da, dc = dev(a), dev(c)
    c_dev0 = dc.clone()
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    comm = costa.Comm.self(0)
    r1, c1 = scales(m, 1, np.float32), scales(n, 2, np.float32)
    r2, c2 = scales(m, 3, np.float32), scales(n, 4, np.float32)
    exp1 = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c, r1, c1)
    exp2 = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c, r2, c2)
    exp0 = c.copy()
    oracle.transform(oracle.FLOAT, op, alpha, beta, a_case.geom(1), [a], c_case.geom(1), [exp0])
    assert len({exp0.tobytes(), exp1.tobytes(), exp2.tobytes()}) == 3
    costa.transform_scaled(A, C, comm, op, alpha, beta, vec(r1), vec(c1))
    assert_bits(host(dc, tc), exp1, tc, "scaled, first vectors")
    dc.copy_(c_dev0)
    costa.transform(A, C, comm, op, alpha, beta)
    assert_bits(host(dc, tc), exp0, tc, "ordinary in between")
    dc.copy_(c_dev0)
    costa.transform_scaled(A, C, comm, op, alpha, beta, vec(r2), vec(c2))
    assert_bits(host(dc, tc), exp2, tc, "scaled, other vectors")


def test_per_channel_quantisation_on_torch_tensors(costa):
    """fp32 -> torch.float8_e4m3fn 'N' with row_scale = 448 / amax per row, the rows' magnitudes a
    different power of two each; then e4m3 -> fp32 'T' with col_scale = amax / 448: both bit-equal to
    the recipe.  One alpha (the mean scale) instead of the vector gives NaN codes."""
    a_case, c_case = geometry("bc203", "N")
    m, n = c_case.shape()
    pw = np.float32(2.0) ** ((np.arange(m) * 7) % 20 - 6).astype(np.float32)
    M = oracle.gen(oracle.FLOAT, 0xB1, 0, m * n).reshape(m, n) * pw[:, None]
    assert M.dtype == np.float32
    a32 = distribute(M, a_case, 1)[0].astype(np.float32)
    amax = np.abs(M).max(axis=1)
    row_scale = (np.float32(448) / amax).astype(np.float32)
    ta = torch.from_numpy(a32).cuda()
    c0 = gen(E4M3, 0xB2, c_case.buf_elems(0, 1))
    tq = torch.from_numpy(c0.copy()).cuda().view(torch.float8_e4m3fn)
    exp = expected_transform(F, E4M3, "N", 1, 0, a_case, c_case, a32, c0, r=row_scale)
    assert_finite(exp, E4M3, "quantise")
    A = make_layout(costa, a_case, 0, ta.data_ptr(), 1, costa.element_code(ta.dtype))
    C = make_layout(costa, c_case, 0, tq.data_ptr(), 1, costa.element_code(tq.dtype))
    comm = costa.Comm.self(0)
    costa.transform_scaled(A, C, comm, "N", 1, 0, row_scale=torch.from_numpy(row_scale).cuda())
    got = tq.view(torch.uint8).cpu().numpy()
    assert_bits(got, exp, E4M3, "per-channel fp32 -> e4m3")
    # the per-tensor scale cannot do this: the mean scale as alpha overflows the large rows
    tq2 = torch.from_numpy(c0.copy()).cuda().view(torch.float8_e4m3fn)
    C2 = make_layout(costa, c_case, 0, tq2.data_ptr(), 1, E4M3)
    costa.transform(A, C2, comm, "N", float(row_scale.mean()), 0)
    assert np.isnan(widen(tq2.view(torch.uint8).cpu().numpy(), E4M3)).any()
    # and back, transposed, into an fp32 tensor: the scale of source row j is col_scale[j]
    t_case, _ = geometry("bc203", "T")  # 157 x 203
    d0 = oracle.gen(oracle.FLOAT, 0xB3, 0, t_case.buf_elems(0, 1))
    td = torch.from_numpy(d0.copy()).cuda()
    col_scale = (amax / np.float32(448)).astype(np.float32)
    exp2 = expected_transform(E4M3, F, "T", 1, 0, c_case, t_case, got.copy(), d0, cs=col_scale)
    assert_finite(exp2, F, "dequantise")
    Tl = make_layout(costa, t_case, 0, td.data_ptr(), 1, costa.element_code(td.dtype))
    costa.transform_scaled(C, Tl, comm, "T", 1, 0, col_scale=torch.from_numpy(col_scale).cuda())
    assert_bits(td.cpu().numpy(), exp2, F, "per-channel e4m3 -> fp32 T")


@pytest.mark.parametrize("geom", ["bc203", "lldpad"])
@pytest.mark.parametrize("code", [F, D], ids=["f32", "f64"])
def test_in_place_equilibration(costa, code, geom):
    """A <- diag(r) * A * diag(c) with A and C the same handle, 'N'; the padding keeps its bytes"""
    _, case = geometry(geom, "N")
    ct = ctype(code, code)
    m, n = case.shape()
    a = gen(code, 0x41, case.buf_elems(0, 1))
    r, cs = scales(m, 0x42, ct), scales(n, 0x43, ct)
    exp = expected_transform(code, code, "N", 1, 0, case, case, a, a.copy(), r, cs)
    assert_finite(exp, code, "in place")
    da = dev(a)
    A = make_layout(costa, case, 0, da.data_ptr(), 1, code)
    costa.transform_scaled(A, A, costa.Comm.self(0), "N", 1, 0, vec(r), vec(cs))
    got = host(da, code)
    assert_bits(got, exp, code, f"in place {NAMES[code]} {geom}")
    pad = distribute(np.ones((m, n)), case, 1)[0] == 0
    assert got[pad].tobytes() == a[pad].tobytes()
    if geom == "lldpad":
        assert pad.any()


# ------------------------------------------------------------------ neighbours
def test_other_transforms_are_unchanged_around_a_scaled_one(costa):
    """an fp32, a bf16 and an e4m3 ordinary transform give identical bytes before and after a scaled
    transform"""
    a_case, c_case = geometry("bc203", "T")
    comm = costa.Comm.self(0)
    data = {code: (gen(code, 0x61 + code, a_case.buf_elems(0, 1)), gen(code, 0x71 + code, c_case.buf_elems(0, 1)))
            for code in (F, BF16, E4M3)}

    def run(code):
        da, dc = dev(data[code][0]), dev(data[code][1])
        costa.transform(make_layout(costa, a_case, 0, da.data_ptr(), 1, code),
                        make_layout(costa, c_case, 0, dc.data_ptr(), 1, code), comm, "T", -0.5, 2.0)
        return dc.cpu().numpy().tobytes()
    before = {code: run(code) for code in data}
    for ta, tc in ((F, F), (BF16, BF16), (E4M3, E4M3)):
        got, exp = _run(costa, ta, tc, "bc203", "T")
        assert_bits(got, exp, tc, "scaled in between")
    after = {code: run(code) for code in data}
    import fp8_common as fc
    import half_common as hc
    exp_f = data[F][1].copy()
    oracle.transform(oracle.FLOAT, "T", -0.5, 2.0, a_case.geom(1), [data[F][0]], c_case.geom(1), [exp_f])
    want = {F: exp_f.tobytes(),
            BF16: hc.expected_transform(BF16, BF16, "T", -0.5, 2.0, a_case, c_case, *data[BF16]).tobytes(),
            E4M3: fc.expected_transform(E4M3, E4M3, "T", -0.5, 2.0, a_case, c_case, *data[E4M3]).tobytes()}
    for code in data:
        assert before[code] == after[code] == want[code], NAMES[code]


# ------------------------------------------------------------------ exchange path
@pytest.mark.parametrize("mode", ["1", "2"])
def test_scaled_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> scaled UNPACK (tests/scaled_loopback_child.py; the mode is
    fixed per process)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scaled_loopback_child.py")
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


# ------------------------------------------------------------------ refusals that need a device
def test_refusals_leave_c_unchanged(costa):
    a_case, c_case = geometry("bc203", "N")
    m, n = c_case.shape()
    comm = costa.Comm.self(0)
    a, c = gen(F, 1, a_case.buf_elems(0, 1)), gen(F, 2, c_case.buf_elems(0, 1))
    r = scales(m, 3, np.float32)
    dr = vec(r)
    # host-resident layouts
    c_host = c.copy()
    A = make_layout(costa, a_case, 0, a.ctypes.data, 1, F)
    C = make_layout(costa, c_case, 0, c_host.ctypes.data, 1, F)
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.transform_scaled(A, C, comm, row_scale=dr)
    assert e.value.code == 1 and c_host.tobytes() == c.tobytes()
    # a host-resident scale vector (a raw host address), and no vector at all
    da, dc = dev(a), dev(c)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, F)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, F)
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.transform_scaled(A, C, comm, row_scale=r.ctypes.data)
    assert e.value.code == 1
    with pytest.raises(costa.CostaError, match="use costa_hip_transform") as e:
        costa.transform_scaled(A, C, comm)
    assert e.value.code == 1
    with pytest.raises(ValueError):
        costa.transform_scaled(A, C, comm, row_scale=vec(scales(m + 1, 3, np.float32)))
    with pytest.raises(ValueError):
        costa.transform_scaled(A, C, comm, row_scale=vec(scales(m, 3, np.float64)))
    assert dc.cpu().numpy().tobytes() == c.tobytes()
    # and the pair works once the vector is on the device
    costa.transform_scaled(A, C, comm, row_scale=dr)
    assert_bits(host(dc, F), expected_transform(F, F, "N", 1, 0, a_case, c_case, a, c, r), F, "after refusals")
