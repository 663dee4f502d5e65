"""MXFP6 without a GPU, part 2: the layout-only half of the quad rule at layout creation, and
costa_hip_plan_export_scaled of the six FP6 pairs -- every op keeps 3-byte groups whole, a pair whose
OTHER layout splits the packed dimension off the grid of 4 is refused ("FP6 quad"), a packed package is
counted in whole bytes, and the MX tile-boundary rule holds on the geometries of the GPU tests."""
import numpy as np
import pytest

import fp6_common as f6
import mx_common as mc
from casegen import BC, Custom
from emulated_ranks import check_geometry
from fp6_common import COLS, E2M3, E3M2, F, FP6, ROWS

GRIDS = {"1x1": (1, 1), "2x2": (2, 2)}
PAIRS = {f"{kind}-{f6.NAMES[p]}": pair
         for p in FP6 for kind, pair in (("quantise", (F, p)), ("dequantise", (p, F)), ("requantise", (p, p)))}
A_BASE, C_BASE = 1 << 40, 1 << 41


def _at(base, code):
    """an FP6 buffer at an odd byte address: no alignment is asked of a block pointer"""
    return base + (3 if code in FP6 else 0)


A_AT, C_AT = _at(A_BASE, E2M3), _at(C_BASE, E2M3)
TYPES = pytest.mark.parametrize("p", FP6, ids=[f6.NAMES[p] for p in FP6])


def _plans(costa, geom, op, grid, ta, tc):
    pm, pn = GRIDS[grid]
    P = pm * pn
    a_case, c_case = f6.geometry(geom, op, (pm, pn))
    out = []
    for r in range(P):
        A = f6.make_layout(costa, a_case, r, _at(A_BASE, ta), P, ta)
        C = f6.make_layout(costa, c_case, r, _at(C_BASE, tc), P, tc)
        out.append(costa.plan_export_scaled(A, C, r, P, op, 1.0, 0.0))
    return a_case, c_case, out


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", f6.GEOMETRIES)
@pytest.mark.parametrize("kind", list(PAIRS))
def test_plans_keep_groups_whole(costa, kind, geom, op, grid):
    ta, tc = PAIRS[kind]
    a_case, c_case, plans = _plans(costa, geom, op, grid, ta, tc)
    P = len(plans)
    m, n = c_case.shape()
    check_geometry(plans)
    A_AT, C_AT = _at(A_BASE, ta), _at(C_BASE, tc)
    assert sum(p.local_scaled.size + p.unpack_scaled.size for p in plans) > 0
    for r, p in enumerate(plans):
        a_bytes, c_bytes = f6.buf_bytes(ta, a_case.buf_elems(r, P)), f6.buf_bytes(tc, c_case.buf_elems(r, P))
        assert p.local_ops.size == 0 and p.unpack_ops.size == 0
        for ops, pkg_src in ((p.local_scaled, False), (p.unpack_scaled, True)):
            for t in ops:
                assert f6.op_quad(t, ta, tc), t
            for axis in (ROWS, COLS):                                  # the MX tile-boundary rule too
                assert mc.boundary_ok(ops, axis, m, n)
            o = ops["op"]
            if ops.size:                                               # byte addresses inside the buffers
                assert (o["dst"] >= C_AT).all() and (o["dst"] < C_AT + c_bytes).all()
                if tc in FP6:                                          # ... on a group boundary of C's buffer
                    assert ((o["dst"].astype(np.int64) - C_AT) % 3 == 0).all()
            if ops.size and not pkg_src:
                assert (o["src"] >= A_AT).all() and (o["src"] < A_AT + a_bytes).all()
                if ta in FP6:
                    assert ((o["src"].astype(np.int64) - A_AT) % 3 == 0).all()
        n_unpack = int((p.unpack_scaled["op"]["nf"].astype(np.int64) * p.unpack_scaled["op"]["ns"]).sum())
        n_pack = int((p.pack_ops["nf"].astype(np.int64) * p.pack_ops["ns"]).sum())
        if ta in FP6:
            # a packed package: counts, displacements and offsets are bytes, 3 per 4 elements; the pack
            # ops are byte copies and tile the send package without a gap
            assert p.recv_elems * 4 == 3 * n_unpack and p.send_elems == n_pack
            u = p.unpack_scaled["op"]
            ends = u["src"].astype(np.int64) + u["nf"].astype(np.int64) * u["ns"] * 3 // 4
            assert u.size == 0 or int(ends.max()) <= p.recv_elems
            assert (u["src"].astype(np.int64) % 3 == 0).all()
            order = np.argsort(p.pack_ops["dst"])
            d = p.pack_ops[order]
            at = 0
            for k in range(d.size):
                assert int(d["dst"][k]) == at
                assert int(d["nf"][k]) % 3 == 0 and int(d["lds"][k]) % 3 == 0    # 3/4 of a multiple of 4
                at += int(d["nf"][k]) * int(d["ns"][k])
            assert at == p.send_elems
            if d.size:  # ... and read whole groups of A's buffer: 3/4 of the extent at 3/4 of the pitch
                last = d["src"].astype(np.int64) + (d["ns"].astype(np.int64) - 1) * d["lds"] + d["nf"]
                assert int(d["src"].min()) >= A_AT and int(last.max()) <= A_AT + a_bytes
                assert ((d["src"].astype(np.int64) - A_AT) % 3 == 0).all()
                a_lds = ({a_case.sizes(P)[0]} if isinstance(a_case, BC)
                         else {ld for _, _, _, ld in a_case._blocks(P)[0][r]})
                assert {int(x) for x in d["lds"]} <= {x * 3 // 4 for x in a_lds}
        else:
            assert p.recv_elems == n_unpack and p.send_elems == n_pack   # fp32 packages count elements
    if grid == "2x2":
        assert any(p.send_elems > 0 for p in plans)


@TYPES
def test_block_pointers_are_byte_addresses(costa, p):
    """a block that starts 64 elements into the local buffer starts 48 bytes into it, at any parity"""
    case = BC(204, 156, 64, 96)
    L = f6.make_layout(costa, case, 0, A_AT, 1, p)
    assert L.shape() == (204, 156) and L.dtype == p
    b0, b1 = L.block(0), L.block(1)
    assert (b0.data, b0.ld) == (A_AT, 204) and (b1.row_start, b1.data) == (64, A_AT + 48)
    b_next_col = [L.block(k) for k in range(L.num_blocks()) if L.block(k).col_start == 96 and L.block(k).row_start == 0]
    assert b_next_col and b_next_col[0].data == A_AT + 96 * 153       # lld 204: a byte pitch of 153, odd
    Fl = case.make_layout(0, A_AT, 1, F)
    assert Fl.block(1).data == A_AT + 64 * 4


@TYPES
def test_layout_creation_accepts_and_refuses(costa, p):
    def bc(m=204, n=156, mb=64, nb=96, i=1, j=1, sub_m=None, sub_n=None, lld=None, ordering="C"):
        sub_m = m - i + 1 if sub_m is None else sub_m
        sub_n = n - j + 1 if sub_n is None else sub_n
        lld = lld if lld is not None else (m if ordering == "C" else n)
        return costa.block_cyclic_layout(m, n, mb, nb, i, j, sub_m, sub_n, 1, 1, "R", 0, 0, A_AT, lld, ordering, 0, p)

    def refused(f, **kw):
        with pytest.raises(costa.CostaError, match="FP6 quad") as ei:
            f(**kw)
        assert ei.value.code == 1 and f6.TYPE_NAMES[p] in str(ei.value), str(ei.value)

    bc()
    bc(lld=208)
    bc(ordering="R")
    bc(m=203, ordering="R")                       # off the grid along the dimension that is NOT packed
    bc(n=155)
    bc(nb=33, lld=204)                            # odd column blocks of a 'C' layout
    bc(i=5, j=2)                                  # a 0-based sub-matrix offset of 4, any column offset
    bc(ordering="R", i=2, j=5)
    refused(bc, lld=206)                          # lld = 2 mod 4
    refused(bc, lld=205)
    refused(bc, m=202, lld=204)                   # extent = 2 mod 4 along the packed dimension
    refused(bc, n=154, ordering="R")
    refused(bc, mb=66)                            # own split point at 66
    refused(bc, nb=66, ordering="R")
    refused(bc, i=3)                              # a 0-based sub-matrix offset of 2
    refused(bc, i=3, sub_m=200)                   # ... with an extent on the grid
    refused(bc, j=3, ordering="R")
    refused(bc, sub_m=102)                        # sub-matrix extent = 2 mod 4

    def custom(rs, cs, ld, ordering="C"):
        return costa.custom_layout(len(rs) - 1, len(cs) - 1, rs, cs, np.zeros((len(rs) - 1, len(cs) - 1), np.int32),
                                   [(A_AT, ld, 0, 0)], ordering, p)
    custom([0, 64, 204], [0, 33, 156], 64)
    custom([0, 65, 203], [0, 32, 156], 32, "R")
    refused(custom, rs=[0, 66, 204], cs=[0, 32, 156], ld=68)
    refused(custom, rs=[0, 64, 204], cs=[0, 32, 156], ld=66)
    refused(custom, rs=[0, 64, 204], cs=[0, 34, 156], ld=36, ordering="R")
    refused(custom, rs=[2, 66, 206], cs=[0, 32, 156], ld=64)   # points off the grid, extents multiples of 4
    # the layout calls stay usable on an FP6 layout (host only)
    L = bc()
    assert L.num_blocks() == 8 and L.shape() == (204, 156)
    L.reorder_ranks([0])


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", list(PAIRS))
def test_a_split_at_66_of_the_other_layout_is_refused(costa, kind, op):
    """the FP6 layout is fine by itself; the other layout cuts its packed dimension at 66 (through op)"""
    ta, tc = PAIRS[kind]
    p = tc if tc in FP6 else ta
    m, n = 204, 156
    one = [[0, 0], [0, 0]]
    quad_c = Custom([0, 64, m], [0, 32, n], one, ord="C")           # 'C': rows are packed
    if kind.startswith("dequantise"):   # A holds FP6; C's grid, seen through op, cuts A's packed rows at 66
        if op == "N":
            a_case, c_case = quad_c, Custom([0, 66, m], [0, 32, n], one, ord="C", ld_pad=1)
        else:                    # A is n x m, its rows are C's columns
            a_case, c_case = Custom([0, 32, n], [0, 64, m], one, ord="C"), Custom([0, 64, m], [0, 66, n], one, ord="C")
    else:                        # C holds FP6 ('C'); A's grid cuts C's packed rows at 66
        c_case = quad_c
        if op == "N":            # (an FP6 A is valid by itself stored 'R': its columns are packed, its rows free)
            a_case = Custom([0, 66, m], [0, 32, n], one, ord="R")
        else:                    # A is n x m, its columns are C's rows; stored 'C' its rows are packed
            a_case = Custom([0, 32, n], [0, 66, m], one, ord="C")
    A = f6.make_layout(costa, a_case, 0, A_AT, 1, ta)
    C = f6.make_layout(costa, c_case, 0, C_AT, 1, tc)
    with pytest.raises(costa.CostaError, match="FP6 quad") as ei:
        costa.plan_export_scaled(A, C, 0, 1, op, 1.0, 0.0)
    msg = str(ei.value)
    assert ei.value.code == 1 and f6.TYPE_NAMES[p] in msg and "[" in msg and "66" in msg   # the offending interval


@TYPES
def test_other_plan_exports_refuse_the_type(costa, p):
    other = E3M2 if p == E2M3 else E2M3
    a_case, c_case = f6.geometry("g204", "N")
    A6 = f6.make_layout(costa, a_case, 0, A_AT, 1, p)
    C6 = f6.make_layout(costa, c_case, 0, C_AT, 1, p)
    Cf = f6.make_layout(costa, c_case, 0, C_AT, 1, F)
    for A, C in ((A6, C6), (A6, Cf)):
        with pytest.raises(costa.CostaError, match=f6.TYPE_NAMES[p]) as ei:
            costa.plan_export([A], [C], 0, 1)
        assert ei.value.code == 1
    # FP6 with a type that is neither itself nor FLOAT has no MX transform, in the scaled export too
    for code in (costa.DOUBLE, costa.HALF, costa.FP8_E4M3, costa.FP4_E2M1, other, costa.INT32, costa.CFLOAT):
        if code in (7, 8):
            Cx = mc.make_layout(costa, c_case, 0, C_AT, 1, code)
        elif code == other:
            Cx = f6.make_layout(costa, c_case, 0, C_AT, 1, code)
        else:
            Cx = c_case.make_layout(0, C_AT, 1, code)
        for A, C in ((A6, Cx), (Cx, C6)):
            with pytest.raises(costa.CostaError, match="no MX transform") as ei:
                costa.plan_export_scaled(A, C, 0, 1)
            assert ei.value.code == 1 and f6.TYPE_NAMES[p] in str(ei.value), str(ei.value)
