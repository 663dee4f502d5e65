"""Scaled transforms without a GPU: the plan (costa_amd.plan_export_scaled) is the ordinary plan with
every LOCAL and UNPACK op moved to the scaled lists, the target coordinates of the scaled ops are
right (checked independently of the planner, by running the lists through the CPU oracle on a
matrix whose values encode their position), unsupported pairs are refused, and the Python surface
matches the header."""
import dataclasses
import types

import numpy as np
import pytest

import oracle
from scaled_common import (BF16, CNAMES, D, E4M3, E5M2, F, F_ROWS, H16, NAMES, PAIR_IDS, PAIRS, geometry,
                           make_layout, op_coords, plain_ops)
from tri_common import distribute, run_plans_cpu

GRIDS = {"1x1": (1, 1), "2x2": (2, 2)}
PLAN_PAIRS = [(F, F), (D, D), (F, E4M3), (E4M3, F), (BF16, BF16)]


def _scalars(op):
    return (1, 0) if op == "N" else (-0.5, 2.0)


# ------------------------------------------------------------------ plan equality
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["bc203", "lldpad", "cfg5"])
@pytest.mark.parametrize("ta,tc", PLAN_PAIRS, ids=[f"{NAMES[a]}-{NAMES[c]}" for a, c in PLAN_PAIRS])
def test_scaled_plan_is_the_ordinary_plan(costa, ta, tc, geom, op, grid):
    pm, pn = GRIDS[grid]
    P = pm * pn
    a_case, c_case = geometry(geom, op, (pm, pn))
    alpha, beta = _scalars(op)
    n_ops = 0
    for r in range(P):
        A = make_layout(costa, a_case, r, 1 << 40, P, ta)
        C = make_layout(costa, c_case, r, 1 << 41, P, tc)
        o = costa.plan_export([A], [C], r, P, [op], [alpha], [beta])
        s = costa.plan_export_scaled(A, C, r, P, op, alpha, beta)
        for f in ("pack_ops", "send_counts", "send_displs", "recv_counts", "recv_displs", "scalars"):
            assert getattr(o, f).tobytes() == getattr(s, f).tobytes(), (r, f)
        assert (o.send_elems, o.recv_elems, o.local_elems) == (s.send_elems, s.recv_elems, s.local_elems)
        # the ordinary local and unpack lists of the scaled plan are empty ...
        assert s.local_ops.size == 0 and s.unpack_ops.size == 0
        # ... and the scaled lists are them, field for field and in order, but for bit 7
        for mine, theirs in ((s.local_scaled, o.local_ops), (s.unpack_scaled, o.unpack_ops)):
            assert mine.size == theirs.size
            assert plain_ops(costa, mine).tobytes() == theirs.tobytes(), r
            assert not (theirs["flags"] & F_ROWS).any()
            n_ops += mine.size
        if P > 1:
            assert s.unpack_scaled.size > 0 and s.pack_ops.size > 0
    assert n_ops > 0


# ------------------------------------------------------------------ coordinates
def _with_ord(case, ordering):
    return dataclasses.replace(case, ord=ordering)


@pytest.mark.parametrize("ords", ["CC", "RC", "CR", "RR"])
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["bc203", "cfg5"])
def test_scaled_op_coordinates(costa, geom, op, grid, ords):
    """DOUBLE, alpha = 1, beta = 0, target M[i, j] = i * 2^20 + j: after the scaled plan's lists ran
    through the oracle as plain tile ops, the destination values at every op's corners decode to the
    (i, j) that row0, col0 and F_ROWS predict"""
    pm, pn = GRIDS[grid]
    P = pm * pn
    a_case, c_case = geometry(geom, op, (pm, pn))
    a_case, c_case = _with_ord(a_case, ords[0]), _with_ord(c_case, ords[1])
    m, n = c_case.shape()
    M = np.arange(m, dtype=np.float64)[:, None] * 2.0 ** 20 + np.arange(n, dtype=np.float64)[None, :]
    a_bufs = distribute(M.T.copy() if op != "N" else M, a_case, P)
    bufs = [(a_bufs[r], np.full(c_case.buf_elems(r, P), -1.0)) for r in range(P)]
    plans, keep = [], []
    for r in range(P):
        A = a_case.make_layout(r, bufs[r][0].ctypes.data, P, oracle.DOUBLE)
        C = c_case.make_layout(r, bufs[r][1].ctypes.data, P, oracle.DOUBLE)
        keep.append((A, C))
        s = costa.plan_export_scaled(A, C, r, P, op, 1, 0)
        plans.append(types.SimpleNamespace(
            pack_ops=s.pack_ops, unpack_ops=plain_ops(costa, s.unpack_scaled),
            local_ops=plain_ops(costa, s.local_scaled), scalars=s.scalars, send_counts=s.send_counts,
            send_displs=s.send_displs, recv_counts=s.recv_counts, recv_displs=s.recv_displs,
            send_elems=s.send_elems, recv_elems=s.recv_elems, scaled=s))
    run_plans_cpu(costa, oracle.DOUBLE, plans, bufs)
    # the whole matrix arrived (the plain ops are a complete redistribution)
    exp = distribute(M, c_case, P)
    seen_rows = seen_cols = 0
    for r in range(P):
        cbuf = bufs[r][1]
        assert (cbuf[cbuf >= 0] == exp[r][cbuf >= 0]).all()
        for t in list(plans[r].scaled.local_scaled) + list(plans[r].scaled.unpack_scaled):
            nf, ns, ldd = int(t["op"]["nf"]), int(t["op"]["ns"]), int(t["op"]["ldd"])
            flags = int(t["op"]["flags"])
            i, j = op_coords(t)
            base = (int(t["op"]["dst"]) - cbuf.ctypes.data) // 8
            for f, s in ((0, 0), (nf - 1, ns - 1)):
                v = int(cbuf[base + (f * ldd + s if flags & 1 else s * ldd + f)])
                assert (v >> 20, v & ((1 << 20) - 1)) == (int(i[f, s]), int(j[f, s])), (r, t, f, s)
            seen_rows += bool(flags & F_ROWS)
            seen_cols += not flags & F_ROWS
    # F_ROWS is the source ordering against the transpose: 'C' != (op != 'N')
    assert (seen_cols == 0) if (ords[0] == "C") != (op != "N") else (seen_rows == 0)


# ------------------------------------------------------------------ refusals
REFUSED = [(2, 2), (3, 3), (4, 4), (F, D), (D, F), (E4M3, E5M2), (E5M2, E4M3), (H16, E4M3), (E4M3, H16)]


@pytest.mark.parametrize("ta,tc", REFUSED, ids=[f"{CNAMES[a]}-{CNAMES[c]}" for a, c in REFUSED])
def test_unsupported_pairs_are_refused_naming_both_types(costa, ta, tc):
    a_case, c_case = geometry("bc203", "N")
    A = make_layout(costa, a_case, 0, 1 << 40, 1, ta)
    C = make_layout(costa, c_case, 0, 1 << 41, 1, tc)
    with pytest.raises(costa.CostaError) as e:
        costa.plan_export_scaled(A, C, 0, 1)
    assert e.value.code == 1  # COSTA_ERR_ARG
    assert f"{CNAMES[ta]} (A)" in str(e.value) and f"{CNAMES[tc]} (C)" in str(e.value), str(e.value)
    with pytest.raises(costa.CostaError) as e:
        costa.scaled_subtile(ta, tc)
    assert e.value.code == 1 and CNAMES[ta] in str(e.value) and CNAMES[tc] in str(e.value)


def test_ordinary_plan_export_is_unchanged_by_a_scaled_one(costa):
    a_case, c_case = geometry("bc203", "T")
    A = make_layout(costa, a_case, 0, 1 << 40, 1, F)
    C = make_layout(costa, c_case, 0, 1 << 41, 1, F)
    before = costa.plan_export([A], [C], 0, 1, ["T"], [-0.5], [2.0])
    costa.plan_export_scaled(A, C, 0, 1, "T", -0.5, 2.0)
    after = costa.plan_export([A], [C], 0, 1, ["T"], [-0.5], [2.0])
    assert before.local_ops.tobytes() == after.local_ops.tobytes() and before.local_ops.size > 0


# ------------------------------------------------------------------ Python surface
def test_python_surface(costa):
    import ctypes
    assert costa.SCALED_OP_DTYPE.itemsize == 48 == ctypes.sizeof(costa.ScaledOp)
    assert costa.SCALED_OP_DTYPE.fields["row0"][1] == 40 and costa.SCALED_OP_DTYPE.fields["col0"][1] == 44
    assert costa.SCALED_F_ROWS == 0x80
    for (ta, tc), name in zip(PAIRS, PAIR_IDS):
        bf, bs = costa.scaled_subtile(ta, tc)
        assert bf > 0 and bs > 0, name
    assert len(PAIRS) == 14
    assert isinstance(costa.scaled_items(), int)
    a_case, _ = geometry("bc203", "N")
    assert make_layout(costa, a_case, 0, 1 << 40, 1, F).shape() == (203, 157)


def test_scale_vector_arguments_are_checked(costa):
    """a tensor argument is checked for dtype, contiguity and length before the native call"""
    torch = pytest.importorskip("torch")
    a_case, c_case = geometry("bc203", "N")
    A = make_layout(costa, a_case, 0, 1 << 40, 1, F)
    C = make_layout(costa, c_case, 0, 1 << 41, 1, F)
    with pytest.raises(ValueError, match="device-resident"):
        costa.transform_scaled(A, C, None, row_scale=torch.ones(203))
    with pytest.raises(ValueError, match="not"):
        costa.transform_scaled(A, C, None, row_scale=np.ones(203, np.float32))
