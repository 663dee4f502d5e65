"""Triangular (masked) transforms on the GPU: the edge-tile kernel (costa_amd/csrc/tri_kernels.hip)
through execute_tiles_tri, and transform_tri through every path of the executor.

Expected values come from the CPU oracle (tri_common.py): the whole op or plan through the oracle,
dropped elements put back.  Every comparison is bit for bit over the whole buffer, so bytes at
dropped positions and in the guard zones around the ops must keep their fill.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from casegen import BC, Custom
from tri_common import (KS, SCALARS, UPLOS, Reference, cases_geometry, kept_of_op, keep_mask,
                        make_plans, oracle_edge_ops, poison_dropped, same_bytes)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S, D, CF, Z, I = oracle.FLOAT, oracle.DOUBLE, oracle.CFLOAT, oracle.CDOUBLE, oracle.INT32
NAMES = {S: "f32", D: "f64", CF: "c64", Z: "c128", I: "i32"}
TR, CONJ, LE = 0x1, 0x2, 0x40
BITCOPY, ZERO, ALPHA, AXPBY = 0, 1, 2, 3


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(oracle.NP[dtype])


# ------------------------------------------------------------------ kernel level
def _edge_list(costa, dtype, transpose, variant):
    """every size x diagonal x sense x scale kind of one (type, mode, alignment) variant as ONE
    list, each op with its own region of the source and destination buffers and 4 elements of
    guard zone around it"""
    bf, bs = costa.tri_subtile(dtype)
    sizes = [(1, 1), (1, 17), (17, 1), (bf + 3, bs + 5), (2 * bf + 1, bs - 1)]
    kinds = [(BITCOPY, 0, 0), (ZERO, 1, 0), (ALPHA, 2, 0), (AXPBY, 3, 0)]
    if dtype in (CF, Z):
        kinds += [(ALPHA, 2, CONJ), (AXPBY, 3, CONJ)]
    rows = []
    src_at = dst_at = 4

    def place(at, fast, slow, shift, odd_ld):
        ld = (fast + 3) // 4 * 4 + (1 if odd_ld else 0)
        first = at + (1 if shift else 0)
        return first, ld, (first + ld * slow + 3) // 4 * 4 + 4

    for nf, ns in sizes:
        # s - f runs over [-(nf - 1), ns - 1]: the diagonal beyond the op on either side, through
        # its corners, through a sub-tile corner, through the middle
        ds = {-(nf - 1) - 3, ns - 1 + 3, -(nf - 1), ns - 1, 0, (ns - nf) // 2 + 1}
        if nf > bf:
            ds |= {bs - bf, -bf, bs - 2 * bf}
        for d in sorted(ds):
            for le in (0, LE):
                for kind, slot, cj in kinds:
                    s0, lds, src_at = place(src_at, nf, ns, variant == "src", variant == "src")
                    df, dslow = (ns, nf) if transpose else (nf, ns)
                    d0, ldd, dst_at = place(dst_at, df, dslow, variant == "dst", variant == "ldd")
                    rows.append((s0, d0, nf, ns, lds, ldd,
                                 (TR if transpose else 0) | cj | le | kind << 4 | slot << 16, 0, d, 0))
    ops = np.array(rows, dtype=costa.TRI_OP_DTYPE)
    return ops, src_at + 4, dst_at + 4


_DTYPES = [S, D, CF, Z, I]


@pytest.mark.parametrize("variant", ["aligned", "dst", "ldd", "src"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("dtype", _DTYPES, ids=[NAMES[t] for t in _DTYPES])
def test_edge_ops(costa, dtype, transpose, variant):
    ops, n_src, n_dst = _edge_list(costa, dtype, transpose, variant)
    E = np.dtype(oracle.NP[dtype]).itemsize
    cplx = dtype in (CF, Z)
    if dtype == I:
        scal = np.array([1, 0, 0, 0, -3, 0, 2, 5], np.int32)
    else:
        scal = np.array([1, 0, 0, 0, -1.5, 0, 0.75 - 0.5j if cplx else 0.75,
                         1.25 + 0.25j if cplx else 1.25], oracle.NP[dtype])
    src = oracle.gen(dtype, 0xA7, 0, n_src)
    dst0 = oracle.gen(dtype, 0xC7, 0, n_dst)  # the sentinel fill of C and of the guard zones
    if dtype != I:  # NaN at every dropped position of A
        for t in ops:
            _, kept = kept_of_op(t)
            f, s = np.nonzero(~kept)
            src[int(t["src"]) + s * int(t["lds"]) + f] = np.nan
    exp = dst0.copy()
    ora = ops.copy()
    ora["src"] = ops["src"] * E
    ora["dst"] = ops["dst"] * E + exp.ctypes.data
    oracle_edge_ops(costa, dtype, ora, scal, exp, src.ctypes.data)
    gpu = ops.copy()
    gpu["src"] = ops["src"] * E
    gpu["dst"] = ops["dst"] * E
    ds, dd = dev(src), dev(dst0)
    items0 = costa.get_stats()["tri_items"]
    costa.execute_tiles_tri(dtype, gpu, scal, ds.data_ptr(), dd.data_ptr())
    got = host(dd, dtype)
    what = f"{NAMES[dtype]} {'T' if transpose else 'N'} {variant}"
    if dtype != I:
        assert not np.isnan(got).any(), what
    if not same_bytes(got, exp):
        bad = np.flatnonzero(got.view(f"V{E}") != exp.view(f"V{E}"))
        k = int(np.searchsorted(ops["dst"], bad[0], side="right")) - 1
        raise AssertionError(f"{what}: {bad.size} elements differ, first at {bad[0]} "
                             f"(op {k}: {ops[k]}): got {got[bad[0]]!r}, expected {exp[bad[0]]!r}")
    # the builder lists exactly the sub-tiles that hold a kept element
    bf, bs = costa.tri_subtile(dtype)
    want_items = 0
    for t in ops:
        _, kept = kept_of_op(t)
        for f0 in range(0, int(t["nf"]), bf):
            for s0 in range(0, int(t["ns"]), bs):
                want_items += bool(kept[f0:f0 + bf, s0:s0 + bs].any())
    assert costa.get_stats()["tri_items"] - items0 == want_items


_SPECIAL_DTYPES = [S, D, CF, Z]


@pytest.mark.parametrize("variant", ["aligned", "dst", "src"])
@pytest.mark.parametrize("transpose", [False, True], ids=["copy", "transpose"])
@pytest.mark.parametrize("dtype", _SPECIAL_DTYPES, ids=[NAMES[t] for t in _SPECIAL_DTYPES])
def test_edge_ops_special_values(costa, dtype, transpose, variant):
    """test_edge_ops' list with oracle.add_specials over the kept positions of A and all of C (the
    dropped positions of A stay NaN): tri_kernel<cpx...> then leaves the vectors whose naive
    products come out NaN in both parts at a kept element to the `redo` blocks of run_tri, which
    must recompute elements klo .. khi of the vector only.  Asserted on the host before the launch,
    from the data and the oracle alone (specials_common.redo_cells): recovered elements in
    sub-tiles that are kept whole and in sub-tiles the diagonal crosses; c64 (two elements a
    vector): a redone vector that straddles the diagonal, a kept flagged element next to a dropped
    one.  Real types have no redo: inf / NaN through the arithmetic, ALPHA / ZERO ops over a C full
    of them.  Every real part of the whole buffer bit-equal or NaN on both sides (at most 15 % of
    the written parts NaN), and every element no op writes -- dropped ones inside redone vectors
    included -- keeps its initial bytes."""
    import specials_common as sc
    ops, n_src, n_dst = _edge_list(costa, dtype, transpose, variant)
    E = np.dtype(oracle.NP[dtype]).itemsize
    cplx = dtype in (CF, Z)
    scal = np.array([1, 0, 0, 0, -1.5, 0, 0.75 - 0.5j if cplx else 0.75,
                     1.25 + 0.25j if cplx else 1.25], oracle.NP[dtype])
    src = oracle.add_specials(oracle.gen(dtype, 0xA7, 0, n_src), dtype, 0xA8, 0)
    dst0 = oracle.add_specials(oracle.gen(dtype, 0xC7, 0, n_dst), dtype, 0xC8, 0)
    for t in ops:  # NaN at every dropped position of A
        _, kept = kept_of_op(t)
        f, s = np.nonzero(~kept)
        src[int(t["src"]) + s * int(t["lds"]) + f] = np.nan
    exp = dst0.copy()
    ora = ops.copy()
    ora["src"] = ops["src"] * E
    ora["dst"] = ops["dst"] * E + exp.ctypes.data
    # (each op as the kind it carries: the list's BITCOPY ops are byte copies in transpose mode too,
    # where the oracle's own rule would multiply by 1)
    oracle_edge_ops(costa, dtype, ora, scal, exp, src.ctypes.data, sc.exec_ops)
    gpu = ops.copy()
    gpu["src"] = ops["src"] * E
    gpu["dst"] = ops["dst"] * E
    what = f"{NAMES[dtype]} {'T' if transpose else 'N'} {variant}"
    kept_of = lambda t: kept_of_op(t)[1]  # noqa: E731
    wr = sc.written(gpu, n_dst, E, kept_of)
    share = sc.assert_nan_share(exp, wr, what)
    assert same_bytes(exp[~wr], dst0[~wr])
    if cplx:
        bf, bs = costa.tri_subtile(dtype)

        def whole_of(t, f0, s0, tf, ts):
            """tri_kernels.hip build_tri_work: a sub-tile is listed when it holds a kept element,
            with the `whole` bit when every element of it is kept"""
            k = kept_of(t)[f0:f0 + tf, s0:s0 + ts]
            return None if not k.any() else bool(k.all())
        cells = sc.redo_cells(sc.strip_subs("tri", gpu, bf, bs, whole_of), src, dst0, exp, scal, 16 // E, kept_of)
        for fill in ("whole", "guarded"):
            for kind in ("ALPHA", "AXPBY"):
                c = sc.total(cells, fill=fill, kind=kind)
                assert c["recovered"] > 0 and c["not_redone"] > 0, f"{what}: {fill} {kind}: {dict(c)}"
        assert sc.total(cells, conj="conj")["recovered"] > 0, what
        if dtype == CF:
            for kind in ("ALPHA", "AXPBY"):
                assert sc.total(cells, kind=kind)["straddle"] > 0, f"{what}: {kind}: no redone vector across the diagonal"
    print(f"{what}: {share:.1%} of the written real parts are NaN")
    ds, dd = dev(src), dev(dst0)
    costa.execute_tiles_tri(dtype, gpu, scal, ds.data_ptr(), dd.data_ptr())
    got = host(dd, dtype)
    sc.assert_parts(got, exp, what)
    assert same_bytes(got[~wr], dst0[~wr]), f"{what}: an element no op writes changed"


# ------------------------------------------------------------------ transform level
OPS = [(D, "N"), (D, "T"), (CF, "N"), (CF, "T"), (CF, "C")]  # ('C' on real types is 'T')
OP_IDS = [f"{NAMES[t]}-{o}" for t, o in OPS]
SHAPES = [(200, 136), (136, 200)]
MASKS = [(u, k) for u in UPLOS for k in KS]


def _run_one_rank(costa, ref, uplo, k, launch=None, poison=False, on_host=False):
    bufs = ref.fresh()
    if poison:
        poison_dropped(bufs, ref.a_case, ref.c_case, 1, ref.op, uplo, k)
    a, c = bufs[0]
    if on_host:
        pa, pc = a.ctypes.data, c.ctypes.data
    else:
        da, dc = dev(a), dev(c)
        pa, pc = da.data_ptr(), dc.data_ptr()
    A = ref.a_case.make_layout(0, pa, 1, ref.dtype)
    C = ref.c_case.make_layout(0, pc, 1, ref.dtype)
    if launch is None:
        costa.transform_tri(A, C, costa.Comm.self(0), ref.op, uplo, k, ref.alpha, ref.beta)
    else:
        launch(A, C)
    return c if on_host else host(dc, ref.dtype)


def _has_edge_ops(costa, ref, uplo, k):
    A = ref.a_case.make_layout(0, 1 << 40, 1, ref.dtype)
    C = ref.c_case.make_layout(0, 1 << 41, 1, ref.dtype)
    p = costa.plan_export_tri(A, C, 0, 1, ref.op, uplo, k, ref.alpha, ref.beta)
    return p.local_tri.size > 0


@pytest.mark.parametrize("dtype,op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["200x136", "136x200"])
def test_transform_tri_one_rank(costa, shape, dtype, op):
    a_case, c_case = cases_geometry(shape, (1, 1), op)
    alpha, beta = SCALARS[dtype]
    ref = Reference(costa, dtype, a_case, c_case, 1, op, alpha, beta)
    for uplo, k in MASKS:
        items0 = costa.get_stats()["tri_items"]
        got = _run_one_rank(costa, ref, uplo, k)
        assert same_bytes(got, ref.expected(uplo, k)[0]), (uplo, k)
        # tri_items > 0 exactly when the plan has edge ops
        assert (costa.get_stats()["tri_items"] > items0) == _has_edge_ops(costa, ref, uplo, k), (uplo, k)
    for uplo, k in (("U", 0), ("L", -1), ("U", -64)):  # NaN at A's dropped positions
        got = _run_one_rank(costa, ref, uplo, k, poison=True)
        assert not np.isnan(got).any(), (uplo, k)
        assert same_bytes(got, ref.expected(uplo, k)[0]), (uplo, k)


@pytest.mark.parametrize("ords", [("C", "C"), ("C", "R"), ("R", "C"), ("R", "R")], ids=lambda o: o[0] + o[1])
@pytest.mark.parametrize("op", ["N", "T"])
def test_transform_tri_band_cut(costa, op, ords):
    n = 2 * costa.tri_cut() + 37
    a_case = Custom([0, n], [0, n], [[0]], ord=ords[0])
    c_case = Custom([0, n], [0, n], [[0]], ord=ords[1], ld_pad=3)
    alpha, beta = SCALARS[D]
    ref = Reference(costa, D, a_case, c_case, 1, op, alpha, beta)
    for uplo, k in (("U", 0), ("L", -1), ("U", 40), ("L", 300)):
        got = _run_one_rank(costa, ref, uplo, k, poison=True)
        assert not np.isnan(got).any(), (uplo, k)
        assert same_bytes(got, ref.expected(uplo, k)[0]), (uplo, k)


def test_keep_all_mask_is_the_ordinary_transform(costa):
    a_case, c_case = cases_geometry((200, 136), (1, 1), "T")
    alpha, beta = SCALARS[D]
    ref = Reference(costa, D, a_case, c_case, 1, "T", alpha, beta)
    comm = costa.Comm.self(0)

    def plain(A, C):
        costa.transform(A, C, comm, "T", alpha, beta)
    want = _run_one_rank(costa, ref, "U", 0, launch=plain)
    assert same_bytes(want, ref.full[0])
    for uplo, k in (("U", -10000), ("L", 10000), ("U", -199), ("L", 135)):
        items0 = costa.get_stats()["tri_items"]
        got = _run_one_rank(costa, ref, uplo, k)
        assert same_bytes(got, want), (uplo, k)
        assert costa.get_stats()["tri_items"] == items0
    for uplo, k in (("U", 10000), ("L", -10000)):  # keeps nothing: a no-op
        assert same_bytes(_run_one_rank(costa, ref, uplo, k), ref.before[0]), (uplo, k)


@pytest.mark.parametrize("dtype,op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("grid", [(2, 2), (2, 3)], ids=["2x2", "2x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=["200x136", "136x200"])
def test_transform_tri_emulated_ranks(costa, shape, grid, dtype, op):
    """every rank's plan on device buffers: PACK through execute_tiles, the exchange by slicing on
    the device, UNPACK and LOCAL through execute_tiles and execute_tiles_tri"""
    P = grid[0] * grid[1]
    a_case, c_case = cases_geometry(shape, grid, op)
    alpha, beta = SCALARS[dtype]
    ref = Reference(costa, dtype, a_case, c_case, P, op, alpha, beta)
    E = np.dtype(oracle.NP[dtype]).itemsize
    for uplo, k in MASKS:
        hb = ref.fresh()
        db = [(dev(a), dev(c)) for a, c in hb]

        class _P:  # what make_plans needs of a buffer: its address
            def __init__(self, t):
                self.ctypes = type("c", (), {"data": t.data_ptr()})
        plans, keep = make_plans(costa, dtype, a_case, c_case, P, [(_P(a), _P(c)) for a, c in db], op,
                                 alpha, beta, uplo, k)
        send = [torch.zeros(max(1, p.send_elems) * E, dtype=torch.uint8, device="cuda") for p in plans]
        recv = [torch.zeros(max(1, p.recv_elems) * E, dtype=torch.uint8, device="cuda") for p in plans]
        for r, p in enumerate(plans):
            if p.pack_ops.size:
                costa.execute_tiles(dtype, p.pack_ops, p.scalars, 0, send[r].data_ptr())
        for r in range(P):
            for q in range(P):
                n = int(plans[r].recv_counts[q])
                assert n == plans[q].send_counts[r]
                d, s = int(plans[r].recv_displs[q]), int(plans[q].send_displs[r])
                recv[r][d * E:(d + n) * E] = send[q][s * E:(s + n) * E]
        for r, p in enumerate(plans):
            if p.unpack_ops.size:
                costa.execute_tiles(dtype, p.unpack_ops, p.scalars, recv[r].data_ptr(), 0)
            if p.local_ops.size:
                costa.execute_tiles(dtype, p.local_ops, p.scalars, 0, 0)
            if p.unpack_tri.size:
                costa.execute_tiles_tri(dtype, p.unpack_tri, p.scalars, recv[r].data_ptr(), 0)
            if p.local_tri.size:
                costa.execute_tiles_tri(dtype, p.local_tri, p.scalars, 0, 0)
        want = ref.expected(uplo, k)
        for r in range(P):
            assert same_bytes(host(db[r][1], dtype), want[r]), (uplo, k, r)
        del keep


def test_transform_tri_async_on_a_torch_stream(costa):
    a_case, c_case = cases_geometry((200, 136), (1, 1), "T")
    alpha, beta = SCALARS[D]
    ref = Reference(costa, D, a_case, c_case, 1, "T", alpha, beta)
    s = torch.cuda.Stream()
    comm = costa.Comm.self(0)

    def launch(A, C):
        with torch.cuda.stream(s):
            costa.transform_tri_async(A, C, comm, "T", "L", -1, alpha, beta, stream=s)
        s.synchronize()
    got = _run_one_rank(costa, ref, "L", -1, launch=launch)
    assert same_bytes(got, ref.expected("L", -1)[0])


@pytest.mark.parametrize("dtype,op", [(D, "N"), (CF, "C")], ids=["f64-N", "c64-C"])
def test_transform_tri_on_host_buffers(costa, dtype, op):
    a_case, c_case = cases_geometry((200, 136), (1, 1), op)
    alpha, beta = SCALARS[dtype]
    ref = Reference(costa, dtype, a_case, c_case, 1, op, alpha, beta)
    for uplo, k in (("U", 0), ("L", -1), ("U", -64), ("L", 10000), ("U", 10000)):
        for ab in ((alpha, beta), (1, 0)):  # beta == 0: dropped elements still keep their bytes
            r2 = ref if ab == (alpha, beta) else Reference(costa, dtype, a_case, c_case, 1, op, *ab)
            got = _run_one_rank(costa, r2, uplo, k, on_host=True)
            assert same_bytes(got, r2.expected(uplo, k)[0]), (uplo, k, ab)


@pytest.mark.parametrize("dtype,op", [(D, "T"), (Z, "C")], ids=["f64-T", "c128-C"])
@pytest.mark.parametrize("uplo,k", [("L", -1), ("U", 1)])
def test_in_place_fill_of_the_other_triangle(costa, dtype, op, uplo, k):
    """A and C are layouts over the SAME device buffer of a 300 x 300 matrix: the strict lower
    (upper) triangle becomes the (conjugate-)transposed strict upper (lower) one; the other
    triangle and the diagonal keep their bytes"""
    n = 300
    case_a, case_c = BC(n, n, 32, 48), BC(n, n, 40, 24)
    m0 = oracle.gen(dtype, 0x31, 0, n * n)
    dm = dev(m0)
    A = case_a.make_layout(0, dm.data_ptr(), 1, dtype)
    C = case_c.make_layout(0, dm.data_ptr(), 1, dtype)
    costa.transform_tri(A, C, costa.Comm.self(0), op, uplo, k)
    got = host(dm, dtype).reshape(n, n, order="F")
    before = m0.reshape(n, n, order="F")
    keep = keep_mask(n, n, uplo, k)
    src = before.T.conj() if op == "C" else before.T
    want = np.where(keep, src, before)
    assert same_bytes(np.asfortranarray(got), np.asfortranarray(want))
    assert same_bytes(got[~keep], before[~keep])


@pytest.mark.parametrize("mode", ["1", "2"])
def test_tri_loopback_exchange(mode):
    """PACK -> ncclSend/ncclRecv to self -> UNPACK of a masked plan, edge tiles included
    (tests/tri_loopback_child.py; the mode is fixed per process)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_loopback_child.py")
    env = dict(os.environ, COSTA_LOOPBACK=mode)
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=180)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, packs, unpacks, tri = out[-1].split()
    assert int(n) >= 6 and int(packs) > 0 and int(unpacks) > 0 and int(tri) > 0, out[-1]


def test_costa_trmr2d_matches_mkl(tmp_path):
    """one process on the GPU: costa_p{s,d,c,z}trmr2d against MKL's p?trmr2d_ on the same inputs
    (tests/scalapack/trmr2d_check.c gpu), the whole local B bit for bit"""
    from test_tri_abi import CONDA, LIB, build_trmr2d_check, run_mpi1
    assert os.path.exists(f"{CONDA}/include/mpi.h") and \
        os.path.exists(os.path.join(LIB, "libcosta_amd_prefixed_scalapack.so")), "MPICH / the shim library"
    r = run_mpi1(build_trmr2d_check(tmp_path, True), "gpu")
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 4 * 3 * 4 + 1
