"""FP8 transforms on the GPU: COSTA_FP8_E4M3 (OCP e4m3fn) and COSTA_FP8_E5M2 (OCP e5m2) layouts,
Q -> Q, FLOAT -> Q and Q -> FLOAT, computed in fp32 with one rounding at the store
(costa_amd/csrc/fp8_kernels.hip; costa_hip.h, "FP8").

The expected value is, in every case, the CPU oracle run in FLOAT on widened inputs with cvt applied
once (fp8_common.py): oracle.transform for transforms, oracle.exec_tile_ops for tile lists; the
casts are torch-CPU's .to(float8 dtype) and .to(float32).  For FLOAT -> Q the oracle reads A
unrounded.  Results are compared as raw bytes over the WHOLE destination buffer, so bytes no op
writes (ld padding, gaps, off-alignment slack) are covered; where the expected value is NaN the
result only has to be a NaN of that type.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from fp8_common import (E4M3, E5M2, ESIZE, F, NAMES, PAIR_IDS, PAIRS, assert_bits, cvt, expected_tiles,
                        expected_transform, gen, geometry, make_layout, widen)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TR = 0x1
BITCOPY, ALPHA, AXPBY = 0, 2, 3
TORCH_DT = {F: torch.float32, E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def host(t, code):
    return t.cpu().numpy().view(np.float32 if code == F else np.uint8)


# ------------------------------------------------------------------ kernel level
# (source shift, destination shift) in elements; a shifted side also has an odd ld.  A 1-byte side
# can be off every vector grid, so 3 matters here.
VARIANTS = {"aligned": (0, 0), "src1": (1, 0), "src2": (2, 0), "src3": (3, 0), "dst1": (0, 1), "dst2": (0, 2),
            "dst3": (0, 3)}


def _tile_list(costa, ta, tc, transpose, variant):
    """Every op size x scale kind of one (pair, mode, alignment) variant as ONE list: each op has
    its own region of the source and of the destination buffer.  Offsets in ELEMENTS.
    -> (ops, source elements, destination elements)"""
    bf, bs = costa.convert_subtile(ta, tc)
    sizes = [(1, 1), (3, 5), (17, 33), (bf + 1, bs + 1), (2 * bf - 1, 7), (7, 2 * bs - 1)]
    kinds = [(ALPHA, 0), (ALPHA, 1), (AXPBY, 2)]
    if ta == tc and not transpose:
        kinds.append((BITCOPY, 0))
    s_off, d_off = VARIANTS[variant]
    ops = np.zeros(len(sizes) * len(kinds), costa.TILE_OP_DTYPE)
    src_at = dst_at = 0

    def place(at, fast, slow, off):
        """region of a fast x slow tile: (first element, ld, next region); regions start on a
        multiple of 16 elements (16 bytes of a 1-byte type, 64 of fp32) and an unshifted tile has
        an ld of a multiple of 16; `off` != 0: the tile starts that many elements later and its ld
        is odd"""
        ld = (fast + 15) // 16 * 16
        if off:
            return at + off, ld + 1, (at + off + (ld + 1) * slow + 15) // 16 * 16
        return at, ld, at + ld * slow

    k = 0
    for nf, ns in sizes:
        for kind, slot in kinds:
            s0, lds, src_at = place(src_at, nf, ns, s_off)
            df, dslow = (ns, nf) if transpose else (nf, ns)
            d0, ldd, dst_at = place(dst_at, df, dslow, d_off)
            ops[k] = (s0, d0, nf, ns, lds, ldd, (TR if transpose else 0) | kind << 4 | slot << 16, 0)
            k += 1
    return ops, src_at + 16, dst_at + 16


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_fp8_kernel_tile_lists(costa, ta, tc, transpose, variant):
    ops, n_src, n_dst = _tile_list(costa, ta, tc, transpose, variant)
    scal = np.array([1, 0, -1.5, 0, 0.75, 1.25], np.float32)
    src, dst0 = gen(ta, 0xA1, n_src), gen(tc, 0xC1, n_dst)
    exp = expected_tiles(ta, tc, ops, scal, src, dst0)
    gpu = ops.copy()
    gpu["src"] = ops["src"] * ESIZE[ta]
    gpu["dst"] = ops["dst"] * ESIZE[tc]
    ds, dd = dev(src), dev(dst0)
    items0 = costa.get_stats()["convert_items"]
    costa.execute_tiles_mixed(ta, tc, gpu, scal, ds.data_ptr(), dd.data_ptr())
    assert_bits(host(dd, tc), exp, tc, f"{NAMES[ta]}->{NAMES[tc]} {'T' if transpose else 'N'} {variant}")
    bf, bs = costa.convert_subtile(ta, tc)
    subs = sum(-(-int(o["nf"]) // bf) * -(-int(o["ns"]) // bs) for o in ops)
    assert costa.get_stats()["convert_items"] - items0 == subs


@pytest.mark.parametrize("code", [E4M3, E5M2], ids=["e4m3", "e5m2"])
def test_qq_bitcopy_keeps_nan_payloads(costa, code):
    """Q -> Q copy mode with alpha = 1, beta = 0 is a byte copy: all 256 codes come out as they
    went in, on the FULL path (a whole sub-tile) and on the guarded one"""
    bf, bs = costa.convert_subtile(code, code)
    nf, ns = bf + 16, bs + 1
    src = np.resize(np.arange(256, dtype=np.uint8), nf * ns)
    ops = np.zeros(1, costa.TILE_OP_DTYPE)
    ops[0] = (0, 0, nf, ns, nf, nf, BITCOPY << 4, 0)
    ds, dd = dev(src), dev(np.zeros(nf * ns, np.uint8))
    costa.execute_tiles_mixed(code, code, ops, np.array([1, 0], np.float32), ds.data_ptr(), dd.data_ptr())
    assert dd.cpu().numpy().tobytes() == src.tobytes()


# ------------------------------------------------------------------ rounding
_LOW16 = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


@pytest.fixture(scope="module")
def rounding_inputs():
    """every fp32 bit pattern whose low 16 bits are one of _LOW16: 393,216 values.  The set holds
    every Q value, every tie between neighbours (subnormal ties and the overflow ties included) and
    the fp32 neighbours of each tie, both signs, zeros, infinities and NaNs."""
    hi = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    bits = (hi[:, None] | np.array(_LOW16, np.uint32)[None, :]).reshape(-1)
    assert bits.size == 393216
    return bits.view(np.float32)


@pytest.mark.parametrize("tc", [E4M3, E5M2], ids=["f32-e4m3", "f32-e5m2"])
def test_narrowing_is_torch_cpu_conversion(costa, tc, rounding_inputs):
    """FLOAT -> Q with alpha = 1, beta = 0 over the rounding set as one column, once as scale kind
    BITCOPY and once as ALPHA (1 * x is exact): torch-CPU's bytes"""
    src = rounding_inputs
    n = src.size
    # the reference conversion does what the contract says at the boundaries
    one = lambda x: int(cvt(np.array([x], np.float32), tc)[0])
    if tc == E4M3:
        assert (one(448.0), one(464.0), one(465.0), one(np.inf), one(-465.0)) == (0x7E, 0x7E, 0x7F, 0x7F, 0xFF)
        assert (one(2.0 ** -9), one(2.0 ** -10), one(1.5 * 2.0 ** -9), one(-0.0)) == (0x01, 0x00, 0x02, 0x80)
    else:
        assert (one(57344.0), one(61439.0), one(61440.0), one(np.inf), one(-61440.0)) == (0x7B, 0x7B, 0x7C, 0x7C, 0xFC)
        assert (one(2.0 ** -16), one(2.0 ** -17), one(1.5 * 2.0 ** -16), one(-0.0)) == (0x01, 0x00, 0x02, 0x80)
    exp1 = cvt(src, tc)
    exp = np.concatenate([exp1, exp1])
    ops = np.zeros(2, costa.TILE_OP_DTYPE)
    ops[0] = (0, 0, n, 1, n, n, BITCOPY << 4, 0)
    ops[1] = (0, n, n, 1, n, n, ALPHA << 4, 0)
    ds, dd = dev(src), dev(np.zeros(2 * n, np.uint8))
    costa.execute_tiles_mixed(F, tc, ops, np.array([1, 0], np.float32), ds.data_ptr(), dd.data_ptr())
    assert_bits(host(dd, tc), exp, tc, f"f32->{NAMES[tc]} rounding set")


@pytest.mark.parametrize("ta", [E4M3, E5M2], ids=["e4m3-f32", "e5m2-f32"])
def test_widening_is_exact_over_all_codes(costa, ta):
    src = np.arange(256, dtype=np.uint8)
    exp = widen(src, ta)
    for flags, nf, ns in ((BITCOPY << 4, 256, 1), (TR | ALPHA << 4, 16, 16)):
        ops = np.zeros(1, costa.TILE_OP_DTYPE)
        ops[0] = (0, 0, nf, ns, nf, ns if flags & TR else nf, flags, 0)
        ds, dd = dev(src), dev(np.zeros(256, np.float32))
        costa.execute_tiles_mixed(ta, F, ops, np.array([1, 0], np.float32), ds.data_ptr(), dd.data_ptr())
        want = exp.reshape(16, 16).T.reshape(-1).copy() if flags & TR else exp
        assert_bits(host(dd, F), want, F, f"{NAMES[ta]}->f32 flags {flags:#x}")


# ------------------------------------------------------------------ transform level
def _scalars(op):
    return (1, 0) if op == "N" else (-0.5, 2.0)


def _run(costa, ta, tc, geom, op, launch=None, seeds=(0x51, 0x52)):
    a_case, c_case = geometry(geom, op)
    alpha, beta = _scalars(op)
    a = gen(ta, seeds[0], a_case.buf_elems(0, 1))
    c = gen(tc, seeds[1], c_case.buf_elems(0, 1))
    exp = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c)
    da, dc = dev(a), dev(c)
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, ta)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc)
    if launch is None:
        costa.transform(A, C, costa.Comm.self(0), op, alpha, beta)
    else:
        launch(A, C, alpha, beta)
    return host(dc, tc), exp


@pytest.mark.parametrize("geom", ["bc203", "whole", "oneblock", "cfg5", "lldpad"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_fp8_transform_matches_oracle(costa, ta, tc, op, geom):
    items0 = costa.get_stats()["convert_items"]
    got, exp = _run(costa, ta, tc, geom, op)
    assert_bits(got, exp, tc, f"{NAMES[ta]}->{NAMES[tc]} {op} {geom}")
    assert costa.get_stats()["convert_items"] > items0


def test_fp8_transform_async_on_a_torch_stream(costa):
    s = torch.cuda.Stream()
    comm = costa.Comm.self(0)

    def launch(A, C, alpha, beta):
        with torch.cuda.stream(s):
            costa.transform_async(A, C, comm, "T", alpha, beta, stream=s)
        s.synchronize()
    got, exp = _run(costa, F, E4M3, "bc203", "T", launch)
    assert_bits(got, exp, E4M3, "async f32->e4m3 T")


def test_fp8_transform_batch_of_two_pairs(costa):
    ta = tc = E5M2
    bufs, exps, As, Cs = [], [], [], []
    specs = [("bc203", "N", 1, 0), ("lldpad", "T", -0.5, 2.0)]
    for k, (geom, op, alpha, beta) in enumerate(specs):
        a_case, c_case = geometry(geom, op)
        a = gen(ta, 0x81 + k, a_case.buf_elems(0, 1))
        c = gen(tc, 0x91 + k, c_case.buf_elems(0, 1))
        exps.append(expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c))
        da, dc = dev(a), dev(c)
        bufs.append((da, dc))
        As.append(make_layout(costa, a_case, 0, da.data_ptr(), 1, ta))
        Cs.append(make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc))
    costa.transform_batch(As, Cs, costa.Comm.self(0), [s[1] for s in specs], [s[2] for s in specs],
                          [s[3] for s in specs])
    for k in range(2):
        assert_bits(host(bufs[k][1], tc), exps[k], tc, f"batch pair {k}")


@pytest.mark.parametrize("code", [E4M3, E5M2], ids=["e4m3", "e5m2"])
def test_fp8_transform_on_torch_fp8_tensors(costa, code):
    """real torch.float8_e4m3fn / torch.float8_e5m2 CUDA tensors, their element type taken from
    tensor.dtype through element_code: quantise fp32 -> Q with alpha = 1 / scale ('N'), dequantise
    Q -> fp32 with alpha = scale ('T')"""
    a_case, c_case = geometry("bc203", "N")
    scale = 64.0
    a32 = (oracle.gen(oracle.FLOAT, 0xB1, 0, a_case.buf_elems(0, 1)) * np.float32(scale)).astype(np.float32)
    ta = torch.from_numpy(a32).cuda()
    c0 = gen(code, 0xB2, c_case.buf_elems(0, 1))
    tq = torch.from_numpy(c0.copy()).cuda().view(TORCH_DT[code])
    assert tq.dtype == TORCH_DT[code] and tq.element_size() == 1
    exp = expected_transform(F, code, "N", 1 / scale, 0, a_case, c_case, a32, c0)
    A = make_layout(costa, a_case, 0, ta.data_ptr(), 1, costa.element_code(ta.dtype))
    C = make_layout(costa, c_case, 0, tq.data_ptr(), 1, costa.element_code(tq.dtype))
    assert (A.dtype, C.dtype) == (F, code)
    comm = costa.Comm.self(0)
    costa.transform(A, C, comm, "N", 1 / scale, 0)
    got = tq.view(torch.uint8).cpu().numpy()
    assert_bits(got, exp, code, "torch fp32 -> fp8 tensor")
    # and back, transposed, into an fp32 tensor: A of the 'T' transform is the 203 x 157 matrix
    # seen as C's layout, its target the 157 x 203 one
    t_case, _ = geometry("bc203", "T")  # 157 x 203
    d0 = oracle.gen(oracle.FLOAT, 0xB3, 0, t_case.buf_elems(0, 1))
    td = torch.from_numpy(d0.copy()).cuda()
    exp2 = expected_transform(code, F, "T", scale, 0, c_case, t_case, got.copy(), d0)
    costa.transform(C, make_layout(costa, t_case, 0, td.data_ptr(), 1, costa.element_code(td.dtype)), comm,
                    "T", scale, 0)
    assert_bits(td.cpu().numpy(), exp2, F, "torch fp8 -> fp32 T")


# ------------------------------------------------------------------ refusals that need a device
def test_fp8_transform_on_host_buffers_is_refused(costa):
    a_case, c_case = geometry("bc203", "N")
    a, c = gen(E4M3, 1, a_case.buf_elems(0, 1)), gen(E4M3, 2, c_case.buf_elems(0, 1))
    A = make_layout(costa, a_case, 0, a.ctypes.data, 1, E4M3)
    C = make_layout(costa, c_case, 0, c.ctypes.data, 1, E4M3)
    with pytest.raises(costa.CostaError, match="device-resident") as e:
        costa.transform(A, C, costa.Comm.self(0))
    assert e.value.code == 1  # COSTA_ERR_ARG
    # an unsupported pair is named before residency is looked at
    C2 = make_layout(costa, c_case, 0, c.ctypes.data, 1, E5M2)
    with pytest.raises(costa.CostaError, match="FP8_E4M3.*FP8_E5M2") as e:
        costa.transform(A, C2, costa.Comm.self(0))
    assert e.value.code == 1


def test_same_type_and_triangular_entry_points_refuse_1_byte_types(costa):
    import ctypes as C_
    a_case, c_case = geometry("bc203", "N")
    da, dc = dev(gen(E4M3, 1, a_case.buf_elems(0, 1))), dev(gen(E4M3, 2, c_case.buf_elems(0, 1)))
    A = make_layout(costa, a_case, 0, da.data_ptr(), 1, E4M3)
    C = make_layout(costa, c_case, 0, dc.data_ptr(), 1, E4M3)
    before = dc.cpu().numpy().tobytes()
    with pytest.raises(costa.CostaError, match="FP8_E4M3") as e:
        costa.transform_tri(A, C, costa.Comm.self(0), "N", "U", 0)
    assert e.value.code == 1
    ops = np.zeros(1, costa.TILE_OP_DTYPE)
    ops[0] = (0, 0, 4, 4, 4, 4, ALPHA << 4, 0)
    lib = costa.lib()
    sc = np.array([1, 0], np.float32)
    one = np.array([1], np.float32)
    for code in (E4M3, E5M2):
        rc = lib.costa_hip_execute_tiles(code, ops.ctypes.data_as(C_.POINTER(costa.TileOp)), 1,
                                         C_.c_void_p(da.data_ptr()), C_.c_void_p(dc.data_ptr()),
                                         sc.ctypes.data, 1, 0)
        assert rc == 1
        tops = np.zeros(1, costa.TRI_OP_DTYPE)
        tops[0] = (0, 0, 4, 4, 4, 4, ALPHA << 4, 0, 0, 0)
        rc = lib.costa_hip_execute_tiles_tri(code, tops.ctypes.data_as(C_.POINTER(costa.TriOp)), 1,
                                             C_.c_void_p(da.data_ptr()), C_.c_void_p(dc.data_ptr()),
                                             sc.ctypes.data, 1, 0)
        assert rc == 1
        rc = lib.costa_hip_copy_and_transform(code, 4, 4, C_.c_void_p(da.data_ptr()), 4, 1,
                                              C_.c_void_p(dc.data_ptr()), 4, 1, 0, 0,
                                              one.ctypes.data_as(C_.c_void_p), one.ctypes.data_as(C_.c_void_p))
        assert rc == 1
    assert dc.cpu().numpy().tobytes() == before


# ------------------------------------------------------------------ GPU planner
@pytest.mark.parametrize("geom", ["cfg5", "bc203"])
@pytest.mark.parametrize("ta,tc", [(E4M3, E4M3), (F, E5M2), (E4M3, F)], ids=["e4m3-e4m3", "f32-e5m2", "e4m3-f32"])
def test_device_planner_matches_host_planner(costa, ta, tc, geom):
    """the GPU planner's lists are byte-equal to the host planner's ('T' with alpha, beta; one rank
    of a 2 x 2 grid, so that the pack and unpack lists and the package offsets take part)"""
    a_case, c_case = geometry(geom, "T", (2, 2))
    A = make_layout(costa, a_case, 1, 1 << 40, 4, ta)
    C = make_layout(costa, c_case, 1, 1 << 41, 4, tc)
    h = costa.plan_export([A], [C], 1, 4, ["T"], [-0.5], [2.0])
    d = costa.plan_export([A], [C], 1, 4, ["T"], [-0.5], [2.0], device=0)
    assert h.local_ops.size > 0 and h.pack_ops.size > 0 and h.unpack_ops.size > 0
    for f in ("local_ops", "pack_ops", "unpack_ops", "send_counts", "send_displs", "recv_counts",
              "recv_displs", "scalars"):
        assert getattr(h, f).tobytes() == getattr(d, f).tobytes(), f
    assert (h.send_elems, h.recv_elems, h.local_elems) == (d.send_elems, d.recv_elems, d.local_elems)


def test_transform_planned_on_the_gpu(costa):
    """with planner mode 2 an FP8 transform is planned on the GPU and gives the oracle's bytes"""
    from casegen import BC
    ta, tc = F, E4M3
    a_case, c_case = BC(256, 256, 4, 4), BC(256, 256, 8, 8)
    a, c = gen(ta, 0x41, a_case.buf_elems(0, 1)), gen(tc, 0x42, c_case.buf_elems(0, 1))
    exp = expected_transform(ta, tc, "T", -0.5, 2.0, a_case, c_case, a, c)
    da, dc = dev(a), dev(c)
    costa.set_planner(2)
    try:
        n0 = costa.get_stats()["device_plans"]
        costa.transform(make_layout(costa, a_case, 0, da.data_ptr(), 1, ta),
                        make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc), costa.Comm.self(0), "T", -0.5, 2.0)
        assert costa.get_stats()["device_plans"] == n0 + 1
    finally:
        costa.set_planner(1)
    assert_bits(host(dc, tc), exp, tc, "planned on the GPU")


# ------------------------------------------------------------------ neighbours
def test_other_transforms_are_unchanged_around_an_fp8_one(costa):
    """an fp32 and a bf16 transform give identical bytes before and after an FP8 transform"""
    import half_common as hc
    a_case, c_case = geometry("bc203", "T")
    comm = costa.Comm.self(0)
    a32 = oracle.gen(oracle.FLOAT, 0x61, 0, a_case.buf_elems(0, 1))
    c32 = oracle.gen(oracle.FLOAT, 0x62, 0, c_case.buf_elems(0, 1))
    a16, c16 = hc.gen(hc.BF16, 0x63, a_case.buf_elems(0, 1)), hc.gen(hc.BF16, 0x64, c_case.buf_elems(0, 1))

    def run(a, c, code):
        da, dc = dev(a), dev(c)
        costa.transform(hc.make_layout(costa, a_case, 0, da.data_ptr(), 1, code),
                        hc.make_layout(costa, c_case, 0, dc.data_ptr(), 1, code), comm, "T", -0.5, 2.0)
        return dc.cpu().numpy().tobytes()
    same0, half0 = run(a32, c32, F), run(a16, c16, hc.BF16)
    got, exp = _run(costa, E4M3, E4M3, "bc203", "T")
    assert_bits(got, exp, E4M3, "fp8 in between")
    same1, half1 = run(a32, c32, F), run(a16, c16, hc.BF16)
    exp_same = c32.copy()
    oracle.transform(oracle.FLOAT, "T", -0.5, 2.0, a_case.geom(1), [a32], c_case.geom(1), [exp_same])
    exp_half = hc.expected_transform(hc.BF16, hc.BF16, "T", -0.5, 2.0, a_case, c_case, a16, c16)
    assert same0 == same1 == exp_same.tobytes()
    assert half0 == half1 == exp_half.tobytes()


# ------------------------------------------------------------------ exchange path
@pytest.mark.parametrize("mode", ["1", "2"])
def test_fp8_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK with A's type in the package
    (tests/fp8_loopback_child.py; the mode is fixed per process)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fp8_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, locals_ = out[-1].split()
    assert int(n) == 6 and int(packs) >= int(n) and int(unpacks) >= int(n), out[-1]
    if mode == "1":
        assert int(locals_) == 0, out[-1]
    else:
        assert int(locals_) > 0, out[-1]
