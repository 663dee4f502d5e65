"""Planner and Python surface of half-precision transforms on the CPU (no GPU needed).

COSTA_HALF / COSTA_BFLOAT16 layouts pair with themselves and with FLOAT (H -> H, FLOAT -> H,
H -> FLOAT).  Such a pair plans exactly like the FLOAT transform of the same geometry: the same ops
in the same order with the same shapes, leading dimensions, scale / transpose / slot bits and
locality hints, the same element offsets on every side, the same counts and displacements.  Only
the byte offsets differ: each side counts in its own element size, the package holds the 2-byte
type, and each side's VEC flag follows its own byte alignment.  The scalars are fp32.
"""
import numpy as np
import pytest

from half_common import BF16, CNAMES, ESIZE, F, H16, PAIR_IDS, PAIRS, geometry, make_layout

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
def test_half_plan_equals_float_plan(costa, ta, tc, op, geom, grid):
    alpha, beta = (1, 0) if op == "N" else (-0.5, 2.0)
    ea, ec, ep = ESIZE[ta], ESIZE[tc], 2
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
        # element offsets: A's side in E_A, C's side in E_C, the package in 2 bytes (it holds H)
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


_REFUSED = [(H16, BF16), (BF16, H16)] + [p for h in (H16, BF16) for o in (1, 2, 3, 4) for p in ((h, o), (o, h))]


@pytest.mark.parametrize("ta,tc", _REFUSED, ids=[f"{CNAMES[a]}-{CNAMES[c]}" for a, c in _REFUSED])
def test_refused_pairs_are_named(costa, ta, tc):
    with pytest.raises(costa.CostaError, match=f"{CNAMES[ta]}.*{CNAMES[tc]}") as e:
        costa.plan_export([_lay(costa, ta, BASE_A)], [_lay(costa, tc, BASE_C)], 0, 1)
    assert e.value.code == 1  # COSTA_ERR_ARG


def test_one_batch_shares_one_pair(costa):
    with pytest.raises(costa.CostaError, match="HALF -> HALF and FLOAT -> HALF") as e:
        costa.plan_export([_lay(costa, H16, BASE_A), _lay(costa, F, BASE_A + (1 << 30))],
                          [_lay(costa, H16, BASE_C), _lay(costa, H16, BASE_C + (1 << 30))], 0, 1)
    assert e.value.code == 1


@pytest.mark.parametrize("t", [H16, BF16], ids=["HALF", "BFLOAT16"])
def test_triangular_plan_with_a_half_type_is_refused(costa, t):
    for ta, tc in ((t, t), (F, t), (t, F)):
        with pytest.raises(costa.CostaError, match=f"{CNAMES[ta]}.*{CNAMES[tc]}") as e:
            costa.plan_export_tri(_lay(costa, ta, BASE_A), _lay(costa, tc, BASE_C), 0, 1, "N", "U", 0)
        assert e.value.code == 1


def test_layouts_of_both_kinds_count_in_elements(costa):
    for code in (H16, BF16):
        L = _lay(costa, code, BASE_A)
        f = _lay(costa, F, BASE_A)
        assert L.dtype == code and L.num_blocks() == f.num_blocks() > 1
        for i in range(L.num_blocks()):
            b, g = L.block(i), f.block(i)
            assert (b.row_start, b.row_end, b.col_start, b.col_end, b.ld) == \
                   (g.row_start, g.row_end, g.col_start, g.col_end, g.ld)
            assert (b.data - BASE_A) * 2 == g.data - BASE_A  # 2-byte elements
        a_case = geometry("cfg5", "N")[0]
        C = make_layout(costa, a_case, 0, BASE_A, 1, code)
        per, _ = a_case._blocks(1)
        assert C.num_blocks() == len(per[0])
        # every block sits at its element offset times 2 bytes (the handle keeps row-major block order
        # or not: compare as sets)
        assert {C.block(i).data for i in range(C.num_blocks())} == {BASE_A + off * 2 for _, _, off, _ in per[0]}
        C.reorder_ranks([0])


def test_python_dtype_surface(costa):
    assert (costa.HALF, costa.BFLOAT16) == (5, 6)
    assert costa.dtype_code(np.float16) == costa.HALF
    assert costa.dtype_code(np.dtype("float16")) == costa.HALF
    assert costa.dtype_code(costa.BFLOAT16) == costa.BFLOAT16
    assert costa.np_dtype(costa.HALF) == np.float16
    assert costa.np_dtype(costa.BFLOAT16) == np.uint16
    # a plain uint16 array is not a bfloat16 matrix
    with pytest.raises(ValueError):
        costa.dtype_code(np.uint16)
    # alpha / beta are packed as fp32 for both codes
    for code in (costa.HALF, costa.BFLOAT16):
        assert costa._scalar_bytes(code, -1.5) == np.float32(-1.5).tobytes()
        assert len(costa._scalar_bytes(code, 1)) == 4


def test_torch_dtype_objects_are_recognised_without_importing_torch(costa):
    """dtype_code goes by the object's module and name"""
    def fake(name):
        cls = type("dtype", (), {"__str__": lambda self: f"torch.{name}", "__repr__": lambda self: f"torch.{name}"})
        cls.__module__ = "torch"
        return cls()
    assert costa.dtype_code(fake("float16")) == costa.HALF
    assert costa.dtype_code(fake("bfloat16")) == costa.BFLOAT16
    assert costa.dtype_code(fake("float32")) == costa.FLOAT
    with pytest.raises(ValueError):
        costa.dtype_code(fake("float8_e4m3fn"))
    try:
        import torch
    except ImportError:
        return
    assert costa.dtype_code(torch.float16) == costa.HALF
    assert costa.dtype_code(torch.bfloat16) == costa.BFLOAT16
    assert costa.dtype_code(torch.float64) == costa.DOUBLE
