"""Block-scaled FP8 transforms without a GPU: the tile-boundary rule on exported scaled plans and on
single ops (costa_hip_block_check_ops against bs_common.boundary_ok), the rules of the descriptor
(costa_hip_block_check_scales), and the scaled plans of the FP8 pairs, which the feature leaves as
they are."""
import numpy as np
import pytest

import bs_common as bc
from bs_common import E4M3, E5M2, F, SHAPES, SHAPE_IDS

GRIDS = {"1x1": (1, 1), "2x2": (2, 2)}


def _plan_ops(costa, geom, op, grid, ta=F, tc=E4M3):
    pm, pn = GRIDS[grid]
    P = pm * pn
    a_case, c_case = bc.geometry(geom, op, (pm, pn))
    out = []
    for r in range(P):
        A = bc.make_layout(costa, a_case, r, 1 << 40, P, ta)
        C = bc.make_layout(costa, c_case, r, 1 << 41, P, tc)
        s = costa.plan_export_scaled(A, C, r, P, op, 1.0, 0.0)
        out += [s.local_scaled, s.unpack_scaled]
    return c_case.shape(), out


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["bc128", "bc128pad", "custom128"])
def test_rule_accepts_layouts_on_multiples_of_128(costa, geom, op, grid):
    (m, n), lists = _plan_ops(costa, geom, op, grid)
    assert (m, n) == (330, 270) and sum(x.size for x in lists) > 0
    for block in SHAPES:
        for ops in lists:
            assert bc.boundary_ok(ops, block, m, n)
            costa.block_check_ops(ops, block, m, n)


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("block", SHAPES, ids=SHAPE_IDS)
def test_rule_refuses_40_by_24_blocks(costa, op, grid, block):
    (m, n), lists = _plan_ops(costa, "bc203", op, grid)
    assert not all(bc.boundary_ok(ops, block, m, n) for ops in lists)
    with pytest.raises(costa.CostaError, match="scale block") as ei:
        for ops in lists:
            costa.block_check_ops(ops, block, m, n)
    assert ei.value.code == 1


def _one(costa, row0, col0, nf, ns, frow=True):
    t = np.zeros(1, costa.SCALED_OP_DTYPE)
    t["op"]["nf"], t["op"]["ns"], t["op"]["lds"], t["op"]["ldd"] = nf, ns, nf, nf
    t["op"]["flags"] = bc.F_ROWS if frow else 0
    t["row0"], t["col0"] = row0, col0
    return t


def test_rule_on_single_ops(costa):
    m, n = 330, 270
    split = _one(costa, 0, 0, 64, 128)                    # rows 0 .. 64: a split at 64
    assert not bc.boundary_ok(split, (128, 128), m, n) and not bc.boundary_ok(split, (128, 1), m, n)
    with pytest.raises(costa.CostaError, match=r"scale block.*rows 0 \.\. 64 of 330"):
        costa.block_check_ops(split, (128, 128), m, n)
    with pytest.raises(costa.CostaError, match="scale block"):
        costa.block_check_ops(split, (128, 1), m, n)
    costa.block_check_ops(split, (1, 128), m, n)          # the same split along the free dimension is fine
    assert bc.boundary_ok(split, (1, 128), m, n)
    ok = [(_one(costa, 256, 256, 74, 14), SHAPES),        # the corner: partial along both
          (_one(costa, 128, 0, 202, 128), SHAPES),        # up to the edge
          (_one(costa, 3, 128, 5, 142), [(1, 128)]), (_one(costa, 128, 7, 128, 9), [(128, 1)]),
          (_one(costa, 5, 128, 128, 9, frow=False), [(1, 128)])]
    for t, shapes in ok:
        for b in shapes:
            assert bc.boundary_ok(t, b, m, n)
            costa.block_check_ops(t, b, m, n)
    bad = [(_one(costa, 64, 0, 128, 128), (128, 128)), (_one(costa, 0, 0, 128, 100), (128, 128)),
           (_one(costa, 0, 64, 1, 128), (1, 128)), (_one(costa, 0, 0, 127, 1), (128, 1)),
           (_one(costa, 0, 128, 100, 9, frow=False), (1, 128))]
    for t, b in bad:
        assert not bc.boundary_ok(t, b, m, n)
        with pytest.raises(costa.CostaError, match="scale block") as ei:
            costa.block_check_ops(t, b, m, n)
        assert ei.value.code == 1
    for shape in ((128, 64), (1, 1), (32, 1), (0, 128), (256, 256)):
        with pytest.raises(costa.CostaError, match="block shape"):
            costa.block_check_ops(_one(costa, 0, 0, 128, 128), shape, m, n)


def _distinct(block, rs, cs, rows, cols):
    nbr, nbc = bc.n_blocks((rows, cols), block)
    at = np.arange(nbr)[:, None] * rs + np.arange(nbc)[None, :] * cs
    return np.unique(at).size == at.size


def test_descriptor_rules(costa):
    rows, cols = 330, 270          # (1,128): 330 x 3 blocks; (128,1): 3 x 270; (128,128): 3 x 3
    D = costa.BlockScales
    ok = [((1, 128), 3, 1), ((1, 128), 1, 330), ((1, 128), 5, 1), ((128, 1), 270, 1), ((128, 1), 1, 3),
          ((128, 128), 3, 1), ((128, 128), 1, 3), ((128, 128), 2, 3), ((128, 1), 2, 3)]
    bad = [((1, 128), 0, 1), ((1, 128), 3, 0), ((1, 128), -3, 1), ((128, 128), 1, 1), ((1, 128), 2, 1),
           ((128, 1), 269, 1), ((128, 128), 2, 2), ((128, 1), 1, 2), ((1, 128), 1, 329)]
    for b, rs, cs in ok:
        assert _distinct(b, rs, cs, rows, cols), (b, rs, cs)
        costa.block_check_scales(D(0, b[0], b[1], rs, cs), rows, cols)
    for b, rs, cs in bad:
        assert rs <= 0 or cs <= 0 or not _distinct(b, rs, cs, rows, cols), (b, rs, cs)
        with pytest.raises(costa.CostaError, match="strides") as ei:
            costa.block_check_scales(D(0, b[0], b[1], rs, cs), rows, cols)
        assert ei.value.code == 1
    for b in ((128, 64), (64, 64), (1, 1), (1, 32), (0, 0), (-128, 128)):
        with pytest.raises(costa.CostaError, match="block shape"):
            costa.block_check_scales(D(0, b[0], b[1], 3, 1), rows, cols)
    with pytest.raises(costa.CostaError, match="4-byte aligned"):
        costa.block_check_scales(D(0x1002, 128, 128, 3, 1), rows, cols)


# what plan_export_scaled gave for the FP8 pairs before the block-scaled entry points existed
# (bc128 'T', one rank of 2 x 2): counts of ops and elements, and a checksum of every list
def _digest(p):
    import zlib
    parts = [p.pack_ops, p.local_scaled, p.unpack_scaled, np.asarray(p.send_counts), np.asarray(p.recv_counts)]
    return (p.local_scaled.size, p.unpack_scaled.size, p.pack_ops.size, int(p.send_elems), int(p.recv_elems),
            zlib.crc32(b"".join(np.ascontiguousarray(x).tobytes() for x in parts)))


GOLDEN = {(F, E4M3): (0, 2, 2, 18176, 32768, 90615681), (E4M3, F): (0, 2, 2, 18176, 32768, 2418634935),
          (E5M2, E5M2): (0, 2, 2, 18176, 32768, 1749791460)}


@pytest.mark.parametrize("pair", [(F, E4M3), (E4M3, F), (E5M2, E5M2)], ids=["f32-e4m3", "e4m3-f32", "e5m2-e5m2"])
def test_scaled_plans_of_the_fp8_pairs_are_unchanged(costa, pair):
    """the block-scaled calls run the cached scaled plan of the pair: its exported form is what an MX or a
    scaled call of the same layouts plans, op for op, whatever rule the block shapes add on top"""
    ta, tc = pair
    a_case, c_case = bc.geometry("bc128", "T", (2, 2))
    A = bc.make_layout(costa, a_case, 1, 1 << 40, 4, ta)
    C = bc.make_layout(costa, c_case, 1, 1 << 41, 4, tc)
    p = costa.plan_export_scaled(A, C, 1, 4, "T", 0.75, 0.0)
    assert _digest(p) == GOLDEN[pair], _digest(p)
    assert p.local_scaled.size + p.unpack_scaled.size > 0
    # every op obeys the rule for every block shape, and the plan's lists tile this rank's part of C
    for ops in (p.local_scaled, p.unpack_scaled):
        for b in SHAPES:
            costa.block_check_ops(ops, b, 330, 270)
    cov = np.zeros((330, 270), int)
    for t in list(p.local_scaled) + list(p.unpack_scaled):
        _, _, i, j = bc.op_index(t)
        cov[i, j] += 1
    assert (cov == bc.owned(c_case, 4, 1)).all()
