"""Planner and Python surface of FP8 transforms on the CPU (no GPU needed).

COSTA_FP8_E4M3 / COSTA_FP8_E5M2 layouts pair with themselves and with FLOAT (Q -> Q, FLOAT -> Q,
Q -> FLOAT).  Such a pair plans exactly like the FLOAT transform of the same geometry: the same ops
in the same order with the same shapes, leading dimensions, scale / transpose / slot bits and
locality hints, the same element offsets on every side, the same counts and displacements.  Only
the byte offsets differ: each side counts in its own element size, the package holds A's type
(1 byte for Q -> Q and Q -> FLOAT, 4 bytes for FLOAT -> Q), and each side's VEC flag follows its own
byte alignment.  The scalars are fp32.
"""
import numpy as np
import pytest

from fp8_common import CNAMES, E4M3, E5M2, ESIZE, F, PAIR_IDS, PAIRS, geometry, make_layout, pkg_code

BASE_A, BASE_C = 1 << 40, 1 << 41
VEC_SRC, VEC_DST = 0x4, 0x8
VEC = VEC_SRC | VEC_DST


def _plan(costa, ta, tc, geom, op, grid, rank, alpha, beta):
    a_case, c_case = geometry(geom, op, grid)
    P = grid[0] * grid[1]
    A = make_layout(costa, a_case, rank, BASE_A, P, ta)
    C = make_layout(costa, c_case, rank, BASE_C, P, tc)
    return costa.plan_export([A], [C], rank, P, [op], [alpha], [beta])


def _elems(v, base, E):
    off = v.astype(np.int64) - base
    assert (off % E == 0).all()
    return off // E


def _vec_ok(ops, e_src, e_dst):
    """each side's VEC flag is set exactly when that side is 16-byte aligned at its own size"""
    src_al = (ops["src"] % 16 == 0) & (ops["lds"].astype(np.int64) * e_src % 16 == 0)
    dst_al = (ops["dst"] % 16 == 0) & (ops["ldd"].astype(np.int64) * e_dst % 16 == 0)
    assert (((ops["flags"] & VEC_SRC) != 0) == src_al).all()
    assert (((ops["flags"] & VEC_DST) != 0) == dst_al).all()


@pytest.mark.parametrize("grid", [(1, 1), (2, 2)], ids=["1rank", "2x2"])
@pytest.mark.parametrize("geom", ["bc203", "lldpad", "cfg5"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=PAIR_IDS)
def test_fp8_plan_equals_float_plan(costa, ta, tc, op, geom, grid):
    alpha, beta = (1, 0) if op == "N" else (-0.5, 2.0)
    ea, ec, ep = ESIZE[ta], ESIZE[tc], ESIZE[pkg_code(ta, tc)]
    assert ep == (4 if ta == F else 1)
    P = grid[0] * grid[1]
    n_pack = n_local = 0
    for rank in range(P):
        mx = _plan(costa, ta, tc, geom, op, grid, rank, alpha, beta)
        fl = _plan(costa, F, F, geom, op, grid, rank, alpha, beta)
        for lst in ("local_ops", "pack_ops", "unpack_ops"):
            m, f = getattr(mx, lst), getattr(fl, lst)
            assert m.size == f.size, lst
            for k in ("nf", "ns", "lds", "ldd", "order"):
                assert (m[k] == f[k]).all(), (lst, k)
            assert ((m["flags"] & ~np.uint32(VEC)) == (f["flags"] & ~np.uint32(VEC))).all(), lst
        # element offsets: A's side in E_A, C's side in E_C, the package in A's element size
        assert (_elems(mx.local_ops["src"], BASE_A, ea) == _elems(fl.local_ops["src"], BASE_A, 4)).all()
        assert (_elems(mx.local_ops["dst"], BASE_C, ec) == _elems(fl.local_ops["dst"], BASE_C, 4)).all()
        assert (_elems(mx.pack_ops["src"], BASE_A, ea) == _elems(fl.pack_ops["src"], BASE_A, 4)).all()
        assert (_elems(mx.pack_ops["dst"], 0, ep) == _elems(fl.pack_ops["dst"], 0, 4)).all()
        assert (_elems(mx.unpack_ops["src"], 0, ep) == _elems(fl.unpack_ops["src"], 0, 4)).all()
        assert (_elems(mx.unpack_ops["dst"], BASE_C, ec) == _elems(fl.unpack_ops["dst"], BASE_C, 4)).all()
        for f in ("send_counts", "send_displs", "recv_counts", "recv_displs"):
            assert (getattr(mx, f) == getattr(fl, f)).all(), f
        assert (mx.send_elems, mx.recv_elems, mx.local_elems) == (fl.send_elems, fl.recv_elems, fl.local_elems)
        # the scalars are fp32 whatever C holds
        assert mx.scalars.dtype == np.float32
        assert mx.scalars[0] == np.float32(alpha) and mx.scalars[1] == np.float32(beta)
        _vec_ok(mx.local_ops, ea, ec)
        _vec_ok(mx.pack_ops, ea, ep)
        _vec_ok(mx.unpack_ops, ep, ec)
        n_pack += mx.pack_ops.size
        n_local += mx.local_ops.size
    assert n_local > 0
    if P > 1:
        assert n_pack > 0


def _lay(costa, t, base):
    return make_layout(costa, geometry("bc203", "N")[0], 0, base, 1, t)


# e4m3 <-> e5m2, and Q with HALF, BFLOAT16, DOUBLE, INT32 or a complex type
_REFUSED = [(E4M3, E5M2), (E5M2, E4M3)] + [p for q in (E4M3, E5M2) for o in (1, 2, 3, 4, 5, 6)
                                           for p in ((q, o), (o, q))]


@pytest.mark.parametrize("ta,tc", _REFUSED, ids=[f"{CNAMES[a]}-{CNAMES[c]}" for a, c in _REFUSED])
def test_refused_pairs_are_named(costa, ta, tc):
    with pytest.raises(costa.CostaError, match=f"{CNAMES[ta]}.*{CNAMES[tc]}") as e:
        costa.plan_export([_lay(costa, ta, BASE_A)], [_lay(costa, tc, BASE_C)], 0, 1)
    assert e.value.code == 1  # COSTA_ERR_ARG


def test_one_batch_shares_one_pair(costa):
    with pytest.raises(costa.CostaError, match="FP8_E4M3 -> FP8_E4M3 and FLOAT -> FP8_E4M3") as e:
        costa.plan_export([_lay(costa, E4M3, BASE_A), _lay(costa, F, BASE_A + (1 << 30))],
                          [_lay(costa, E4M3, BASE_C), _lay(costa, E4M3, BASE_C + (1 << 30))], 0, 1)
    assert e.value.code == 1
    with pytest.raises(costa.CostaError, match="FP8_E5M2 -> FLOAT and FP8_E4M3 -> FLOAT") as e:
        costa.plan_export([_lay(costa, E5M2, BASE_A), _lay(costa, E4M3, BASE_A + (1 << 30))],
                          [_lay(costa, F, BASE_C), _lay(costa, F, BASE_C + (1 << 30))], 0, 1)
    assert e.value.code == 1


@pytest.mark.parametrize("t", [E4M3, E5M2], ids=["FP8_E4M3", "FP8_E5M2"])
def test_triangular_plan_with_a_1_byte_type_is_refused(costa, t):
    for ta, tc in ((t, t), (F, t), (t, F)):
        with pytest.raises(costa.CostaError, match=f"{CNAMES[ta]}.*{CNAMES[tc]}") as e:
            costa.plan_export_tri(_lay(costa, ta, BASE_A), _lay(costa, tc, BASE_C), 0, 1, "N", "U", 0)
        assert e.value.code == 1


def test_layouts_of_both_kinds_count_in_elements(costa):
    for code in (E4M3, E5M2):
        L = _lay(costa, code, BASE_A)
        f = _lay(costa, F, BASE_A)
        assert L.dtype == code and L.num_blocks() == f.num_blocks() > 1
        for i in range(L.num_blocks()):
            b, g = L.block(i), f.block(i)
            assert (b.row_start, b.row_end, b.col_start, b.col_end, b.ld) == \
                   (g.row_start, g.row_end, g.col_start, g.col_end, g.ld)
            assert (b.data - BASE_A) * 4 == g.data - BASE_A  # 1-byte elements
        a_case = geometry("cfg5", "N")[0]
        C = make_layout(costa, a_case, 0, BASE_A, 1, code)
        per, _ = a_case._blocks(1)
        assert C.num_blocks() == len(per[0])
        # every block sits at its element offset times 1 byte (compared as sets: the handle may
        # reorder its blocks)
        assert {C.block(i).data for i in range(C.num_blocks())} == {BASE_A + off for _, _, off, _ in per[0]}
        assert len({off for _, _, off, _ in per[0]}) > 1
        C.reorder_ranks([0])


def _fake_torch_dtype(name):
    cls = type("dtype", (), {"__str__": lambda self: f"torch.{name}", "__repr__": lambda self: f"torch.{name}"})
    cls.__module__ = "torch"
    return cls()


def test_python_dtype_surface(costa):
    assert (costa.FP8_E4M3, costa.FP8_E5M2) == (7, 8)
    assert costa.np_dtype(costa.FP8_E4M3) == np.uint8
    assert costa.np_dtype(costa.FP8_E5M2) == np.uint8
    # alpha / beta are packed as fp32 for both codes, on either side of a pair
    for code in (costa.FP8_E4M3, costa.FP8_E5M2):
        assert costa._scalar_bytes(code, -1.5) == np.float32(-1.5).tobytes()
        assert len(costa._scalar_bytes(code, 1)) == 4
        assert costa._scalar_code(code, code) == costa.FLOAT
        assert costa._scalar_code(costa.FLOAT, code) == costa.FLOAT
        assert costa._scalar_code(code, costa.FLOAT) == costa.FLOAT
    assert costa._scalar_code(costa.FLOAT, costa.DOUBLE) == costa.DOUBLE


def test_element_code_knows_the_fp8_types_and_dtype_code_does_not(costa):
    """element_code goes by the object's module and name, without importing torch"""
    assert costa.element_code(_fake_torch_dtype("float8_e4m3fn")) == costa.FP8_E4M3
    assert costa.element_code(_fake_torch_dtype("float8_e5m2")) == costa.FP8_E5M2
    # ... and accepts everything dtype_code accepts
    assert costa.element_code(_fake_torch_dtype("bfloat16")) == costa.BFLOAT16
    assert costa.element_code(_fake_torch_dtype("float32")) == costa.FLOAT
    assert costa.element_code(np.float16) == costa.HALF
    assert costa.element_code(np.dtype("complex128")) == costa.CDOUBLE
    assert costa.element_code(costa.FP8_E5M2) == costa.FP8_E5M2
    # a plain uint8 array is not an FP8 matrix; other FP8 flavours are not supported
    with pytest.raises(ValueError):
        costa.element_code(np.uint8)
    with pytest.raises(ValueError):
        costa.element_code(_fake_torch_dtype("float8_e4m3fnuz"))
    # dtype_code is as it was
    with pytest.raises(ValueError):
        costa.dtype_code(_fake_torch_dtype("float8_e4m3fn"))
    with pytest.raises(ValueError):
        costa.dtype_code(np.uint8)
    try:
        import torch
    except ImportError:
        return
    assert costa.element_code(torch.float8_e4m3fn) == costa.FP8_E4M3
    assert costa.element_code(torch.float8_e5m2) == costa.FP8_E5M2
    assert costa.element_code(torch.float64) == costa.DOUBLE
    with pytest.raises(ValueError):
        costa.dtype_code(torch.float8_e4m3fn)


def test_layout_constructors_and_subtile_helper_take_fp8_dtype_objects(costa):
    a_case = geometry("bc203", "N")[0]
    L = a_case.make_layout(0, BASE_A, 1, _fake_torch_dtype("float8_e4m3fn"))
    assert L.dtype == costa.FP8_E4M3
    # every FP8 pair reports one sub-tile shape, (Q, Q) included
    shapes = {costa.convert_subtile(a, c) for a, c in PAIRS}
    assert len(shapes) == 1
    bf, bs = shapes.pop()
    assert bf > 0 and bs > 0
    assert costa.convert_subtile(_fake_torch_dtype("float8_e5m2"), np.float32) == (bf, bs)
    with pytest.raises(costa.CostaError, match="FP8_E4M3.*FP8_E5M2") as e:
        costa.convert_subtile(E4M3, E5M2)
    assert e.value.code == 1
