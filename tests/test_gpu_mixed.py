"""Mixed-precision transforms on the GPU: sub(C) = beta*sub(C) + alpha*op(convert(sub(A))) with
A and C of different element types (fp64 <-> fp32, c128 <-> c64), the conversion fused into the
tile kernels (costa_amd/csrc/convert_kernels.hip).

The expected value is, in every case, the existing CPU oracle run in C's type on inputs that were
converted first (numpy astype = the C++ static_cast): oracle.transform for transforms,
oracle.exec_tile_ops for tile lists.  Results are compared as raw bit patterns; where the
expected value is NaN the result only has to be NaN (payloads of converted NaNs are not compared).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from casegen import BC, Custom

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S, D, CF, Z = oracle.FLOAT, oracle.DOUBLE, oracle.CFLOAT, oracle.CDOUBLE
PAIRS = [(D, S), (S, D), (Z, CF), (CF, Z)]
NAMES = {S: "f32", D: "f64", CF: "c64", Z: "c128"}
PAIR_IDS = [f"{NAMES[a]}-{NAMES[c]}" for a, c in PAIRS]
ESIZE = {S: 4, D: 8, CF: 8, Z: 16}
TR, CONJ = 0x1, 0x2
BITCOPY, ALPHA, AXPBY = 0, 2, 3


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def convert(a, code):
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(oracle.NP[code])


def assert_bits(got, exp, what):
    """bit-for-bit, except that an expected NaN only asks for a NaN"""
    rt = np.float32 if exp.dtype in (np.float32, np.complex64) else np.float64
    ut = np.uint32 if rt == np.float32 else np.uint64
    g, e = got.view(rt), exp.view(rt)
    nan = np.isnan(e)
    assert np.isnan(g[nan]).all(), f"{what}: NaN expected"
    bad = np.flatnonzero((g.view(ut) != e.view(ut)) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} reals differ, first at {bad[0]}: "
                           f"got {g[bad[0]]!r}, expected {e[bad[0]]!r}")


# ------------------------------------------------------------------ kernel level
def _tile_list(ta, tc, transpose, variant):
    """Every op size x scale kind of one (pair, mode, alignment) variant as ONE list: each op has
    its own region of the source and of the destination buffer.  -> (GPU ops, oracle ops whose
    source offsets count in C's type, source elements, destination elements)"""
    import costa_amd as costa
    bf, bs = costa.convert_subtile(ta, tc)
    sizes = [(1, 1), (3, 5), (bf + 1, bs + 1), (2 * bf - 1, 7), (7, 2 * bs - 1)]
    kinds = [(ALPHA, 0, 0), (ALPHA, 1, 0), (AXPBY, 2, 0)]
    if tc in (CF, Z):
        kinds += [(ALPHA, 1, CONJ), (AXPBY, 2, CONJ)]
    es, ed = ESIZE[ta], ESIZE[tc]
    gpu = np.zeros(len(sizes) * len(kinds), costa.TILE_OP_DTYPE)
    src_at = dst_at = 0

    def place(at, fast, slow, odd):
        """region of a fast x slow tile: (first element, ld, next region); `odd`: one element off
        a 16-byte boundary, odd ld"""
        ld = (fast + 3) // 4 * 4
        if odd:
            return at + 1, ld + 1, (at + 1 + (ld + 1) * slow + 3) // 4 * 4
        return at, ld, at + ld * slow

    k = 0
    for nf, ns in sizes:
        for kind, slot, cj in kinds:
            s0, lds, src_at = place(src_at, nf, ns, variant == "src")
            df, dslow = (ns, nf) if transpose else (nf, ns)
            d0, ldd, dst_at = place(dst_at, df, dslow, variant == "dst")
            gpu[k] = (s0 * es, d0 * ed, nf, ns, lds, ldd,
                      (TR if transpose else 0) | cj | kind << 4 | slot << 16, 0)
            k += 1
    ora = gpu.copy()
    ora["src"] = gpu["src"] // es * ed
    return gpu, ora, src_at + 4, dst_at + 4


@pytest.mark.parametrize("variant", ["aligned", "src", "dst"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_convert_kernel_tile_lists(costa, ta, tc, transpose, variant):
    gpu, ora, n_src, n_dst = _tile_list(ta, tc, transpose, variant)
    cplx = tc in (CF, Z)
    scal = np.array([1, 0, -1.5, 0, 0.75 - 0.5j if cplx else 0.75, 1.25 + 0.25j if cplx else 1.25],
                    oracle.NP[tc])
    src = oracle.gen(ta, 0xA1, 0, n_src)
    dst0 = oracle.gen(tc, 0xC1, 0, n_dst)
    exp = dst0.copy()
    conv = convert(src, tc)
    oracle.exec_tile_ops(tc, ora, scal, conv.ctypes.data, exp.ctypes.data)
    ds, dd = dev(src), dev(dst0)
    items0 = costa.get_stats()["convert_items"]
    costa.execute_tiles_mixed(ta, tc, gpu, scal, ds.data_ptr(), dd.data_ptr())
    got = dd.cpu().numpy().view(oracle.NP[tc])
    assert_bits(got, exp, f"{NAMES[ta]}->{NAMES[tc]} {'T' if transpose else 'N'} {variant}")
    bf, bs = costa.convert_subtile(ta, tc)
    subs = sum(-(-int(o["nf"]) // bf) * -(-int(o["ns"]) // bs) for o in gpu)
    assert costa.get_stats()["convert_items"] - items0 == subs


_SPECIAL_CASES = [pytest.param(ta, tc, sc, id=f"{NAMES[ta]}-{NAMES[tc]}-{sc}")
                  for ta, tc in PAIRS for sc in ("drawn", "huge") if sc == "drawn" or tc in (CF, Z)]


@pytest.mark.parametrize("variant", ["aligned", "src", "dst"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc,scalars", _SPECIAL_CASES)
def test_convert_kernel_tile_lists_special_values(costa, ta, tc, transpose, variant, scalars):
    """test_convert_kernel_tile_lists' list with oracle.add_specials over source and destination:
    convert_kernel<cpx...> then leaves the strips whose naive products come out NaN in both parts to
    the `redo` blocks of run_convert (copy: source and destination read again; transpose: the
    staged tile of the narrower type), next to strips it stores as usual.  Asserted on the host
    before the launch, from the data and the oracle alone (specials_common.redo_cells): the whole
    sub-tile of the (bf + 1) x (bs + 1) ops and the guarded ones each hold a recovered element under
    ALPHA and AXPBY, plain and CONJ; "huge" (alpha = 1e30 + 1e30i, or 1e300 + 1e300i where C is c128):
    recoveries without an infinite input, the overflow branch.  The real pairs have no redo: inf /
    NaN through conv, and ALPHA ops must not read a C full of them.  Every real part bit-equal or NaN
    on both sides, at most 15 % of the written parts NaN."""
    import specials_common as sc
    gpu, ora, n_src, n_dst = _tile_list(ta, tc, transpose, variant)
    cplx = tc in (CF, Z)
    scal = np.array([1, 0, -1.5, 0, 0.75 - 0.5j if cplx else 0.75, 1.25 + 0.25j if cplx else 1.25],
                    oracle.NP[tc])
    if scalars == "huge":
        a, b = sc.HUGE[np.dtype(oracle.NP[tc])]
        scal[2:] = (a, 0, a, b)
    src = oracle.add_specials(oracle.gen(ta, 0xA1, 0, n_src), ta, 0xA5, 0)
    dst0 = oracle.add_specials(oracle.gen(tc, 0xC1, 0, n_dst), tc, 0xC5, 0)
    exp = dst0.copy()
    conv = convert(src, tc)
    # (the oracle, each op as the kind it carries: the list's ALPHA op with alpha = 1 is a product on
    # copy ops too, where the oracle's own rule would memcpy)
    sc.exec_ops(tc, ora, scal, conv.ctypes.data, exp.ctypes.data)
    what = f"{NAMES[ta]}->{NAMES[tc]} {'T' if transpose else 'N'} {variant} {scalars}"
    share = sc.assert_nan_share(exp, sc.written(ora, n_dst, ESIZE[tc]), what)
    bf, bs = costa.convert_subtile(ta, tc)
    if cplx:
        # strip_work.hpp strip_alignment: 16 bytes on the c128 side, 8 on the c64 side, so both VEC
        # flags hold for every op and a sub-tile is whole exactly when it is bf x bs; a strip of
        # cshape is 8 bytes of the narrower type: one element
        subs = sc.strip_subs("convert", ora, bf, bs, lambda op, f0, s0, tf, ts: tf == bf and ts == bs)
        cells = sc.redo_cells(subs, conv, dst0, exp, scal, 1)
        for fill in ("whole", "guarded"):
            for kind in ("ALPHA", "AXPBY"):
                for cj in ("plain", "conj"):
                    c = sc.total(cells, fill=fill, kind=kind, conj=cj)
                    assert c["recovered"] > 0 and c["not_redone"] > 0, f"{what}: {fill} {kind} {cj}: {dict(c)}"
        if scalars == "huge":
            # (AXPBY: beta * y overflows on C's own 3e38 / 1e308; a c128 source's 1e308 is inf once
            # converted to c64, so ALPHA ops overflow only where the source is c64)
            for kind in ("ALPHA", "AXPBY") if tc == Z else ("AXPBY",):
                assert sc.total(cells, kind=kind)["overflow"] > 0, f"{what}: {kind}: no overflow-branch recovery"
    print(f"{what}: {share:.1%} of the written real parts are NaN")
    ds, dd = dev(src), dev(dst0)
    costa.execute_tiles_mixed(ta, tc, gpu, scal, ds.data_ptr(), dd.data_ptr())
    got = dd.cpu().numpy().view(oracle.NP[tc])
    sc.assert_parts(got, exp, what)


def _rounding_values():
    flt_max = float(np.finfo(np.float32).max)
    half = flt_max + 2.0 ** 103          # halfway between FLT_MAX and 2^128: ties to even = inf
    below = np.nextafter(half, 0.0)      # the largest double that still rounds to FLT_MAX
    v = [1.0 + 2.0 ** -24,               # tie, even neighbour below: -> 1
         1.0 + 3 * 2.0 ** -24,           # tie, even neighbour above: -> 1 + 2^-22
         1.0 + 2.0 ** -24 + 2.0 ** -52,  # just above a tie
         2.0 ** -140,                    # an fp32 subnormal, kept
         2.0 ** -149, 2.0 ** -150,       # the smallest subnormal; a tie that rounds to 0
         1.5 * 2.0 ** -149,              # a tie between subnormals 1 and 2: -> 2 * 2^-149
         1e-50, 1e39, -0.0, 0.0, np.inf, -np.inf, below, half, flt_max, 1.0 / 3.0]
    v = v + [-x for x in v]
    with np.errstate(over="ignore"):
        assert np.float32(below) == np.float32(flt_max) and np.isinf(np.float32(half))
    return np.array(v, np.float64)


@pytest.mark.parametrize("ta,tc", [(D, S), (Z, CF)], ids=["f64-f32", "c128-c64"])
def test_narrowing_rounds_like_static_cast(costa, ta, tc):
    """one op of 64 elements, convert only: ties in both parities, subnormals, underflow,
    overflow, signed zeros, infinities and the FLT_MAX boundary, bit for bit with astype"""
    vals = _rounding_values()
    n = 64
    if ta == D:
        src = np.resize(vals, n)
    else:
        src = np.empty(n, np.complex128)
        src.real, src.imag = np.resize(vals, n), np.resize(np.roll(vals, 7), n)
    src = np.ascontiguousarray(src, oracle.NP[ta])
    exp = convert(src, tc)
    scal = np.array([1, 0], oracle.NP[tc])
    # scale kind BITCOPY of a converting op = convert only (a scaled complex op would turn
    # inf + 0i into inf + NaN i, as the same-type kernels do); as one column, and as an 8 x 8
    # transpose through the staged tile
    for flags, nf, ns in ((BITCOPY << 4, n, 1), (TR | BITCOPY << 4, 8, 8)):
        ops = np.zeros(1, costa.TILE_OP_DTYPE)
        ops[0] = (0, 0, nf, ns, nf, ns if flags & TR else nf, flags, 0)
        ds, dd = dev(src), dev(np.zeros(n, oracle.NP[tc]))
        costa.execute_tiles_mixed(ta, tc, ops, scal, ds.data_ptr(), dd.data_ptr())
        got = dd.cpu().numpy().view(oracle.NP[tc])
        want = exp.reshape(8, 8).T.reshape(-1).copy() if flags & TR else exp
        assert_bits(got, want, f"{NAMES[ta]}->{NAMES[tc]} flags {flags:#x}")


# ------------------------------------------------------------------ transform level
def _cfg5_small(op):
    """the ragged custom layouts of the golden cfg5 cases (tests/golden/cases.py), on one rank"""
    from cases import _edges
    m, n = 2048, 1920
    am, an = (n, m) if op != "N" else (m, n)
    ars, acs = _edges(0xC5A1, am, 8, 96), _edges(0xC5A2, an, 8, 96)
    crs, ccs = _edges(0xC5A3, m, 16, 160), _edges(0xC5A4, n, 16, 160)
    return (Custom(ars, acs, np.zeros((len(ars) - 1, len(acs) - 1), np.int32)),
            Custom(crs, ccs, np.zeros((len(crs) - 1, len(ccs) - 1), np.int32)))


def _geometry(name, op):
    t = op != "N"

    def dims(m, n):
        return (n, m) if t else (m, n)
    if name == "bc203":
        return BC(*dims(203, 157), 32, 48), BC(203, 157, 40, 24)
    if name == "whole":
        return BC(256, 256, 128, 128), BC(256, 256, 128, 128)
    if name == "oneblock":
        am, an = dims(300, 260)
        return BC(am, an, am, an), BC(300, 260, 64, 64)
    if name == "cfg5":
        return _cfg5_small(op)
    if name == "lldpad":
        return BC(*dims(203, 157), 32, 48, lld_pad=1), BC(203, 157, 40, 24, lld_pad=1)
    raise KeyError(name)


def _scalars(tc, op):
    if op == "N":
        return 1, 0
    return (0.75 - 0.5j, 1.25 + 0.25j) if tc in (CF, Z) else (-0.5, 2.0)


def _run(costa, ta, tc, a_case, c_case, op, alpha, beta, launch=None):
    a = oracle.gen(ta, 0x51, 0, a_case.buf_elems(0, 1))
    c = oracle.gen(tc, 0x52, 0, c_case.buf_elems(0, 1))
    exp = c.copy()
    oracle.transform(tc, op, alpha, beta, a_case.geom(1), [convert(a, tc)], c_case.geom(1), [exp])
    da, dc = dev(a), dev(c)
    A = a_case.make_layout(0, da.data_ptr(), 1, ta)
    C = c_case.make_layout(0, dc.data_ptr(), 1, tc)
    if launch is None:
        costa.transform(A, C, costa.Comm.self(0), op, alpha, beta)
    else:
        launch(A, C)
    return dc.cpu().numpy().view(oracle.NP[tc]), exp


_TRANSFORMS = [pytest.param(ta, tc, op, id=f"{NAMES[ta]}-{NAMES[tc]}-{op}")
               for ta, tc in PAIRS for op in ("N", "T", "C") if op != "C" or tc in (CF, Z)]


@pytest.mark.parametrize("geom", ["bc203", "whole", "oneblock", "cfg5", "lldpad"])
@pytest.mark.parametrize("ta,tc,op", _TRANSFORMS)
def test_mixed_transform_matches_oracle(costa, ta, tc, op, geom):
    a_case, c_case = _geometry(geom, op)
    alpha, beta = _scalars(tc, op)
    items0 = costa.get_stats()["convert_items"]
    got, exp = _run(costa, ta, tc, a_case, c_case, op, alpha, beta)
    assert_bits(got, exp, f"{NAMES[ta]}->{NAMES[tc]} {op} {geom}")
    if geom in ("bc203", "whole"):
        assert costa.get_stats()["convert_items"] > items0


def test_mixed_transform_async_on_a_torch_stream(costa):
    a_case, c_case = _geometry("bc203", "T")
    s = torch.cuda.Stream()
    comm = costa.Comm.self(0)

    def launch(A, C):
        with torch.cuda.stream(s):
            costa.transform_async(A, C, comm, "T", -0.5, 2.0, stream=s)
        s.synchronize()
    got, exp = _run(costa, D, S, a_case, c_case, "T", -0.5, 2.0, launch)
    assert_bits(got, exp, "async f64->f32 T")


def test_mixed_transform_on_host_buffers_is_refused(costa):
    a_case, c_case = _geometry("bc203", "N")
    a = oracle.gen(D, 1, 0, a_case.buf_elems(0, 1))
    c = oracle.gen(S, 2, 0, c_case.buf_elems(0, 1))
    A = a_case.make_layout(0, a.ctypes.data, 1, D)
    C = c_case.make_layout(0, c.ctypes.data, 1, S)
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.transform(A, C, costa.Comm.self(0))
    assert e.value.code == 1  # COSTA_ERR_ARG


def test_same_type_transforms_are_unchanged_around_a_mixed_one(costa):
    a_case, c_case = _geometry("bc203", "T")
    a = oracle.gen(D, 0x61, 0, a_case.buf_elems(0, 1))
    c = oracle.gen(D, 0x62, 0, c_case.buf_elems(0, 1))
    comm = costa.Comm.self(0)

    def same_type():
        da, dc = dev(a), dev(c)
        costa.transform(a_case.make_layout(0, da.data_ptr(), 1, D),
                        c_case.make_layout(0, dc.data_ptr(), 1, D), comm, "T", -0.5, 2.0)
        return dc.cpu().numpy().tobytes()
    items0 = costa.get_stats()["convert_items"]
    before = same_type()
    assert costa.get_stats()["convert_items"] == items0
    got, exp = _run(costa, D, S, a_case, c_case, "T", -0.5, 2.0)
    assert_bits(got, exp, "mixed in between")
    items1 = costa.get_stats()["convert_items"]
    assert items1 > items0
    after = same_type()
    assert costa.get_stats()["convert_items"] == items1
    exp_same = c.copy()
    oracle.transform(D, "T", -0.5, 2.0, a_case.geom(1), [a], c_case.geom(1), [exp_same])
    assert before == after == exp_same.tobytes()


# ------------------------------------------------------------------ exchange path
@pytest.mark.parametrize("mode", ["1", "2"])
def test_mixed_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK with the narrower type in the package
    (tests/mixed_loopback_child.py; the mode is fixed per process)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mixed_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_ = out[-1].split()
    assert int(n) == 4 and int(packs) >= int(n) and int(unpacks) >= int(n), out[-1]
    if mode == "1":
        assert int(locals_) == 0, out[-1]
    else:
        assert int(locals_) > 0, out[-1]
