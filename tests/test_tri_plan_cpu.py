"""Planner of triangular (masked) transforms on the CPU (no GPU needed).

costa_amd.plan_export_tri for every rank; ordinary ops through the oracle, edge ops through the
oracle with the dropped elements restored, the exchange by slicing (tri_common.py).  The result
must equal where(mask, C_full, C_before) bit for bit, C_full being the ordinary plan through the
oracle.
"""
import numpy as np
import pytest

import oracle
from casegen import BC, Custom
from tri_common import (KS, SCALARS, UPLOS, Reference, cases_geometry, keep_mask, make_plans,
                        poison_dropped, run_plans_cpu, same_bytes)

D, CF = oracle.DOUBLE, oracle.CFLOAT
SHAPES = [(200, 136), (136, 200)]
GRIDS = [(1, 1), (2, 2), (2, 3)]
OPS = [(D, "N"), (D, "T"), (CF, "N"), (CF, "T"), (CF, "C")]  # ('C' on real types is 'T')
BASE_A, BASE_C = 1 << 40, 1 << 41


def _check_masks(costa, ref, masks, poison=False):
    for uplo, k in masks:
        bufs = ref.fresh()
        if poison:
            poison_dropped(bufs, ref.a_case, ref.c_case, ref.P, ref.op, uplo, k)
        plans, keep = make_plans(costa, ref.dtype, ref.a_case, ref.c_case, ref.P, bufs, ref.op,
                                 ref.alpha, ref.beta, uplo, k)
        run_plans_cpu(costa, ref.dtype, plans, bufs)
        want = ref.expected(uplo, k)
        for r in range(ref.P):
            got = bufs[r][1]
            assert same_bytes(got, want[r]), (uplo, k, r, int((got != want[r]).sum()))
            if poison:
                assert not np.isnan(got).any(), (uplo, k, r)
        del keep


@pytest.mark.parametrize("dtype,op", OPS, ids=[f"{'d' if t == D else 'c'}{o}" for t, o in OPS])
@pytest.mark.parametrize("grid", GRIDS, ids=["1x1", "2x2", "2x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=["200x136", "136x200"])
def test_masked_plan_matches_masked_oracle(costa, shape, grid, dtype, op):
    a_case, c_case = cases_geometry(shape, grid, op)
    alpha, beta = SCALARS[dtype]
    ref = Reference(costa, dtype, a_case, c_case, grid[0] * grid[1], op, alpha, beta)
    _check_masks(costa, ref, [(u, k) for u in UPLOS for k in KS])


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("grid", [(1, 1), (2, 2)], ids=["1x1", "2x2"])
def test_nan_at_dropped_positions_does_not_leak(costa, grid, op):
    a_case, c_case = cases_geometry((200, 136), grid, op)
    for alpha, beta in (SCALARS[D], (0.0, 2.0)):  # also alpha == 0
        ref = Reference(costa, D, a_case, c_case, grid[0] * grid[1], op, alpha, beta)
        _check_masks(costa, ref, [("U", 0), ("L", -1), ("U", -64)], poison=True)


@pytest.mark.parametrize("ords", [("C", "C"), ("C", "R"), ("R", "C"), ("R", "R")],
                         ids=lambda o: o[0] + o[1])
@pytest.mark.parametrize("op", ["N", "T"])
def test_single_block_band_cut(costa, op, ords):
    """one block of side 2*tri_cut() + 37: three row bands, each one edge tile and one ordinary"""
    n = 2 * costa.tri_cut() + 37
    a_case = Custom([0, n], [0, n], [[0]], ord=ords[0])
    c_case = Custom([0, n], [0, n], [[0]], ord=ords[1], ld_pad=3)
    alpha, beta = SCALARS[D]
    ref = Reference(costa, D, a_case, c_case, 1, op, alpha, beta)
    _check_masks(costa, ref, [("U", 0), ("L", -1), ("U", 40), ("L", 300)])
    A = a_case.make_layout(0, BASE_A, 1, D)
    C = c_case.make_layout(0, BASE_C, 1, D)
    p = costa.plan_export_tri(A, C, 0, 1, op, "U", 0, alpha, beta)
    cut = costa.tri_cut()
    assert p.local_tri.size == 3 and p.local_ops.size == 3 and p.unpack_tri.size == 0
    for t in p.local_tri:  # an edge tile is narrower than its band is tall
        assert min(int(t["nf"]), int(t["ns"])) <= cut - 1 and max(int(t["nf"]), int(t["ns"])) <= cut
    kept = sum(int(o["nf"]) * int(o["ns"]) for o in p.local_ops)
    from tri_common import kept_of_op
    kept += sum(int(kept_of_op(t)[1].sum()) for t in p.local_tri)
    assert kept == int(keep_mask(n, n, "U", 0).sum()) == p.local_elems


def _pair(costa, grid=(1, 1), rank=0, dt=D, m=200, n=136):
    P = grid[0] * grid[1]
    a = BC(m, n, 32, 48, pm=grid[0], pn=grid[1])
    c = BC(m, n, 40, 24, pm=grid[0], pn=grid[1])
    return a.make_layout(rank, BASE_A, P, dt), c.make_layout(rank, BASE_C, P, dt), P


@pytest.mark.parametrize("grid", [(1, 1), (2, 2)], ids=["1x1", "2x2"])
def test_keep_all_is_the_ordinary_plan_and_keep_nothing_is_empty(costa, grid):
    for rank in range(grid[0] * grid[1]):
        A, C, P = _pair(costa, grid, rank)
        full = costa.plan_export([A], [C], rank, P, ["N"], [2.0], [0.5])
        for uplo, k in (("U", -10000), ("L", 10000), ("U", -199), ("L", 135)):
            p = costa.plan_export_tri(A, C, rank, P, "N", uplo, k, 2.0, 0.5)
            assert p.local_tri.size == 0 and p.unpack_tri.size == 0
            for f in ("local_ops", "pack_ops", "unpack_ops", "send_counts", "send_displs",
                      "recv_counts", "recv_displs", "scalars"):
                assert getattr(p, f).tobytes() == getattr(full, f).tobytes(), (uplo, k, f)
            assert (p.send_elems, p.recv_elems, p.local_elems) == \
                   (full.send_elems, full.recv_elems, full.local_elems)
        for uplo, k in (("U", 10000), ("L", -10000), ("U", 136), ("L", -200)):
            p = costa.plan_export_tri(A, C, rank, P, "N", uplo, k, 2.0, 0.5)
            for f in ("local_ops", "pack_ops", "unpack_ops", "local_tri", "unpack_tri"):
                assert getattr(p, f).size == 0, (uplo, k, f)
            assert (p.send_elems, p.recv_elems, p.local_elems) == (0, 0, 0)
            assert not p.send_counts.any() and not p.recv_counts.any()


def test_exchange_volume_counts_only_rectangles_with_a_kept_element(costa):
    """N = 1024, nb = 64 on 2 x 2, 'U' k = 0; C's grid starts one process row later (rsrc = 1), so
    every block changes owner.  A rank sends exactly the elements of the (A tile) x (C tile)
    rectangles that hold a kept element (the diagonal passes through the corners of the blocks it
    meets, so no column of such a rectangle is wholly dropped)."""
    N, nb, P = 1024, 64, 4
    a = BC(N, N, nb, nb, pm=2, pn=2)
    c = BC(N, N, nb, nb, pm=2, pn=2, rsrc=1)
    keep = keep_mask(N, N, "U", 0)
    want = np.zeros((P, P), np.int64)
    for bi in range(N // nb):
        for bj in range(N // nb):
            src = (bi % 2) * 2 + bj % 2
            dst = ((bi + 1) % 2) * 2 + bj % 2
            rect = keep[bi * nb:(bi + 1) * nb, bj * nb:(bj + 1) * nb]
            if src != dst and rect.any():
                want[src, dst] += rect.size
    assert want.sum() > 0
    for rank in range(P):
        A = a.make_layout(rank, BASE_A, P, D)
        C = c.make_layout(rank, BASE_C, P, D)
        p = costa.plan_export_tri(A, C, rank, P, "N", "U", 0)
        assert (p.send_counts == want[rank]).all(), (rank, p.send_counts, want[rank])
        assert (p.recv_counts == want[:, rank]).all()
        assert p.send_elems == want[rank].sum() and p.recv_elems == want[:, rank].sum()
        full = costa.plan_export([A], [C], rank, P)
        assert full.send_elems == N * N // P and p.send_elems < 0.6 * full.send_elems


def test_errors(costa):
    A, C, P = _pair(costa)
    for bad in ("A", "X", "0"):
        with pytest.raises(costa.CostaError, match="uplo") as e:
            costa.plan_export_tri(A, C, 0, 1, "N", bad, 0)
        assert e.value.code == 1
    costa.plan_export_tri(A, C, 0, 1, "N", "u", 0)  # case-insensitive
    costa.plan_export_tri(A, C, 0, 1, "N", "l", 0)
    S = BC(200, 136, 32, 48).make_layout(0, BASE_A, 1, oracle.FLOAT)
    with pytest.raises(costa.CostaError, match="one element type.*FLOAT.*DOUBLE") as e:
        costa.plan_export_tri(S, C, 0, 1, "N", "U", 0)
    assert e.value.code == 1
    with pytest.raises(costa.CostaError, match="batches") as e:
        costa.plan_export_tri([A, A], [C, C], 0, 1, "N", "U", 0)
    assert e.value.code == 1
    with pytest.raises(costa.CostaError, match="batches"):
        costa.transform_tri([A], [C], None, "N", "U", 0)
