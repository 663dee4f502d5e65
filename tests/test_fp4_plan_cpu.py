"""MXFP4 without a GPU, part 2: the layout-only half of the evenness rule at layout creation, and
costa_hip_plan_export_scaled of the three FP4 pairs -- every op keeps bytes whole, a pair whose OTHER
layout splits the packed dimension at an odd point is refused ("FP4 pair"), a packed package is counted
in whole bytes, and the MX tile-boundary rule holds on the geometries of the GPU tests."""
import numpy as np
import pytest

import fp4_common as f4
import mx_common as mc
from casegen import BC, Custom
from emulated_ranks import check_geometry
from fp4_common import COLS, F, FP4, ROWS

GRIDS = {"1x1": (1, 1), "2x2": (2, 2)}
PAIRS = {"quantise": (F, FP4), "dequantise": (FP4, F), "requantise": (FP4, FP4)}
A_AT, C_AT = 1 << 40, 1 << 41


def _plans(costa, geom, op, grid, ta, tc):
    pm, pn = GRIDS[grid]
    P = pm * pn
    a_case, c_case = f4.geometry(geom, op, (pm, pn))
    out = []
    for r in range(P):
        A = f4.make_layout(costa, a_case, r, A_AT, P, ta)
        C = f4.make_layout(costa, c_case, r, C_AT, P, tc)
        out.append(costa.plan_export_scaled(A, C, r, P, op, 1.0, 0.0))
    return a_case, c_case, out


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["g202", "g202pad", "custom32"])
@pytest.mark.parametrize("kind", list(PAIRS))
def test_plans_keep_bytes_whole(costa, kind, geom, op, grid):
    ta, tc = PAIRS[kind]
    a_case, c_case, plans = _plans(costa, geom, op, grid, ta, tc)
    P = len(plans)
    m, n = c_case.shape()
    check_geometry(plans)
    assert sum(p.local_scaled.size + p.unpack_scaled.size for p in plans) > 0
    for r, p in enumerate(plans):
        assert p.local_ops.size == 0 and p.unpack_ops.size == 0
        for ops, pkg_src in ((p.local_scaled, False), (p.unpack_scaled, True)):
            for t in ops:
                assert f4.op_even(t, ta, tc), t
            for axis in (ROWS, COLS):                                  # the MX tile-boundary rule too
                assert mc.boundary_ok(ops, axis, m, n)
            o = ops["op"]
            if tc == FP4 and ops.size:                                 # destinations: byte addresses inside C's buffer
                assert (o["dst"] >= C_AT).all() and (o["dst"] < C_AT + c_case.buf_elems(r, P) // 2).all()
            if ta == FP4 and ops.size and not pkg_src:
                assert (o["src"] >= A_AT).all() and (o["src"] < A_AT + a_case.buf_elems(r, P) // 2).all()
        n_unpack = int((p.unpack_scaled["op"]["nf"].astype(np.int64) * p.unpack_scaled["op"]["ns"]).sum())
        n_pack = int((p.pack_ops["nf"].astype(np.int64) * p.pack_ops["ns"]).sum())
        if ta == FP4:
            # a packed package: counts, displacements and offsets are bytes, two elements each; the pack
            # ops are byte copies and tile the send package without a gap
            assert p.recv_elems * 2 == n_unpack and p.send_elems == n_pack
            u = p.unpack_scaled["op"]
            ends = u["src"].astype(np.int64) + u["nf"].astype(np.int64) * u["ns"] // 2
            assert u.size == 0 or int(ends.max()) <= p.recv_elems
            order = np.argsort(p.pack_ops["dst"])
            d = p.pack_ops[order]
            at = 0
            for k in range(d.size):
                assert int(d["dst"][k]) == at
                at += int(d["nf"][k]) * int(d["ns"][k])
            assert at == p.send_elems
            if d.size:  # ... and read whole bytes of A's buffer: half the extent, half the pitch
                last = d["src"].astype(np.int64) + (d["ns"].astype(np.int64) - 1) * d["lds"] + d["nf"]
                assert int(d["src"].min()) >= A_AT and int(last.max()) <= A_AT + a_case.buf_elems(r, P) // 2
        else:
            assert p.recv_elems == n_unpack and p.send_elems == n_pack   # fp32 packages count elements
    if grid == "2x2":
        assert any(p.send_elems > 0 for p in plans)


def test_block_pointers_are_byte_addresses(costa):
    """a block that starts 64 elements into the local buffer starts 32 bytes into it"""
    case = BC(202, 158, 64, 96)
    L = f4.make_layout(costa, case, 0, A_AT, 1, FP4)
    assert L.shape() == (202, 158) and L.dtype == FP4
    b0, b1 = L.block(0), L.block(1)
    assert (b0.data, b0.ld) == (A_AT, 202) and (b1.row_start, b1.data) == (64, A_AT + 32)
    Fl = case.make_layout(0, A_AT, 1, F)
    assert Fl.block(1).data == A_AT + 64 * 4


def test_layout_creation_accepts_and_refuses(costa):
    def bc(m=202, n=158, mb=64, nb=96, i=1, j=1, sub_m=None, sub_n=None, lld=None, ordering="C"):
        sub_m = m - i + 1 if sub_m is None else sub_m
        sub_n = n - j + 1 if sub_n is None else sub_n
        lld = lld if lld is not None else (m if ordering == "C" else n)
        return costa.block_cyclic_layout(m, n, mb, nb, i, j, sub_m, sub_n, 1, 1, "R", 0, 0, A_AT, lld, ordering, 0, FP4)

    def refused(f, **kw):
        with pytest.raises(costa.CostaError, match="FP4 pair") as ei:
            f(**kw)
        assert ei.value.code == 1 and "FP4_E2M1" in str(ei.value), str(ei.value)

    bc()
    bc(lld=204)
    bc(ordering="R")
    bc(m=203, ordering="R")                       # odd along the dimension that is NOT packed
    bc(nb=33, lld=202)                            # odd column blocks of a 'C' layout
    bc(i=3, j=2)                                  # even row offset (0-based 2), any column offset
    bc(ordering="R", i=2, j=3)
    refused(bc, lld=203)                          # odd lld
    refused(bc, m=203)                            # odd extent along the packed dimension
    refused(bc, n=157, ordering="R")
    refused(bc, mb=33)                            # odd own split point
    refused(bc, nb=33, ordering="R")
    refused(bc, i=2)                              # odd sub-matrix offset (0-based 1)
    refused(bc, j=2, ordering="R")
    refused(bc, sub_m=101)                        # odd sub-matrix extent

    def custom(rs, cs, ld, ordering="C"):
        return costa.custom_layout(len(rs) - 1, len(cs) - 1, rs, cs, np.zeros((len(rs) - 1, len(cs) - 1), np.int32),
                                   [(A_AT, ld, 0, 0)], ordering, FP4)
    custom([0, 64, 202], [0, 33, 158], 64)
    custom([0, 65, 203], [0, 32, 158], 32, "R")
    refused(custom, rs=[0, 65, 202], cs=[0, 32, 158], ld=66)
    refused(custom, rs=[0, 64, 202], cs=[0, 32, 158], ld=65)
    refused(custom, rs=[0, 64, 202], cs=[0, 33, 158], ld=34, ordering="R")
    refused(custom, rs=[1, 65, 203], cs=[0, 32, 158], ld=64)   # odd split points, even extents
    # the layout calls stay usable on an FP4 layout (host only)
    L = bc()
    assert L.num_blocks() == 8 and L.shape() == (202, 158)
    L.reorder_ranks([0])


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", list(PAIRS))
def test_an_odd_split_of_the_other_layout_is_refused(costa, kind, op):
    """the FP4 layout is fine by itself; the other layout cuts its packed dimension at 65 (through op)"""
    ta, tc = PAIRS[kind]
    m, n = 202, 158
    one = [[0, 0], [0, 0]]
    even_c = Custom([0, 64, m], [0, 32, n], one, ord="C")           # 'C': rows are packed
    if kind == "dequantise":     # A holds FP4; C's grid, seen through op, cuts A's packed rows at an odd point
        if op == "N":
            a_case, c_case = even_c, Custom([0, 65, m], [0, 32, n], one, ord="C", ld_pad=1)
        else:                    # A is n x m, its rows are C's columns
            a_case, c_case = Custom([0, 32, n], [0, 64, m], one, ord="C"), Custom([0, 64, m], [0, 33, n], one, ord="C")
    else:                        # C holds FP4 ('C'); A's grid cuts C's packed rows at 65
        c_case = even_c
        if op == "N":            # (an FP4 A is valid by itself stored 'R': its columns are packed, its rows free)
            a_case = Custom([0, 65, m], [0, 32, n], one, ord="R")
        else:                    # A is n x m, its columns are C's rows; stored 'C' its rows are packed
            a_case = Custom([0, 32, n], [0, 65, m], one, ord="C")
    A = f4.make_layout(costa, a_case, 0, A_AT, 1, ta)
    C = f4.make_layout(costa, c_case, 0, C_AT, 1, tc)
    with pytest.raises(costa.CostaError, match="FP4 pair") as ei:
        costa.plan_export_scaled(A, C, 0, 1, op, 1.0, 0.0)
    assert ei.value.code == 1 and "[" in str(ei.value)          # the offending interval


def test_other_plan_exports_refuse_the_type(costa):
    a_case, c_case = f4.geometry("g202", "N")
    A4 = f4.make_layout(costa, a_case, 0, A_AT, 1, FP4)
    C4 = f4.make_layout(costa, c_case, 0, C_AT, 1, FP4)
    Cf = f4.make_layout(costa, c_case, 0, C_AT, 1, F)
    for A, C in ((A4, C4), (A4, Cf)):
        with pytest.raises(costa.CostaError, match="FP4_E2M1") as ei:
            costa.plan_export([A], [C], 0, 1)
        assert ei.value.code == 1
    # FP4 with a type that is neither FP4 nor FLOAT has no MX transform, in the scaled export too
    for code in (costa.DOUBLE, costa.HALF, costa.FP8_E4M3, costa.INT32, costa.CFLOAT):
        Cx = mc.make_layout(costa, c_case, 0, C_AT, 1, code) if code in (7, 8) else c_case.make_layout(0, C_AT, 1, code)
        with pytest.raises(costa.CostaError, match="FP4_E2M1") as ei:
            costa.plan_export_scaled(A4, Cx, 0, 1)
        assert ei.value.code == 1
