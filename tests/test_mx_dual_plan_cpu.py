"""Dual-output MX quantise without a GPU (costa_hip.h, "Dual-output MX quantise"):
costa_hip_plan_export_dual.  Every exported dual op maps source element (f, s) through dst2 / ldd2 / flags2
to the address of Ct's element (j, i), the ops of all ranks cover Ct exactly once (which also settles that
the flipped rank-grid ordering transposes the owners), and the twin rule, the block rule of either output
and the packed rules on Ct's side are refused with their messages."""
import numpy as np
import pytest

import mx_common as mc
import mx_dual_common as dc
import mx_sr_common as sr
from casegen import BC, Custom
from mx_dual_common import E2M3, E4M3, F, FP4, GEOM_IDS, GEOMS, NAMES

GRIDS = {"1x1": (1, 1), "2x2": (2, 2)}
A_AT, C_AT, CT_AT = 1 << 40, 1 << 41, 1 << 42
TR, F_ROWS = 0x1, 0x80


def _layouts(costa, tq, a_case, c_case, ct_case, r, P):
    lay = sr.family(tq)[2]
    return (lay(costa, a_case, r, A_AT, P, F), lay(costa, c_case, r, C_AT, P, tq), lay(costa, ct_case, r, CT_AT, P, tq))


@pytest.mark.parametrize("ct_ord", ["C", "R"])
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("tq,geom", GEOMS, ids=GEOM_IDS)
def test_twin_addresses(costa, tq, geom, op, grid, ct_ord):
    pm, pn = GRIDS[grid]
    P = pm * pn
    a_case, c_case = dc.geometry(tq, geom, op, (pm, pn))
    ct_case = dc.twin(c_case, ct_ord)
    m, n = c_case.shape()
    assert ct_case.shape() == (n, m)
    # Ct's buffers hold the id of the element they store: id(row, col) = row * m + col + 1 < 2^24
    ids = (np.arange(n)[:, None] * m + np.arange(m)[None, :] + 1).astype(np.float32)
    assert ids.max() < 2 ** 24
    held = mc.place(ct_case, P, ids, [np.zeros(ct_case.buf_elems(r, P), np.float32) for r in range(P)])
    seen = np.zeros((n, m), np.int64)
    n_ops = 0
    for r in range(P):
        A, C, Ct = _layouts(costa, tq, a_case, c_case, ct_case, r, P)
        p = costa.plan_export_dual(A, C, Ct, r, P, op, 1.0, c_axis="rows", ct_axis="rows")
        p2 = costa.plan_export_dual(A, C, Ct, r, P, op, 1.0, c_axis="cols", ct_axis="cols")
        s = costa.plan_export_scaled(A, C, r, P, op, 1.0, 0.0)
        # the scaled plan of (A, C, trans), op for op
        assert p.local_dual["s"].tobytes() == s.local_scaled.tobytes()
        assert p.unpack_dual["s"].tobytes() == s.unpack_scaled.tobytes()
        assert p2.local_dual.tobytes() == p.local_dual.tobytes() and p.send_elems == s.send_elems
        for d in list(p.local_dual) + list(p.unpack_dual):
            n_ops += 1
            nf, ns = int(d["s"]["op"]["nf"]), int(d["s"]["op"]["ns"])
            f, sidx = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
            frow = bool(int(d["s"]["op"]["flags"]) & F_ROWS)
            i = int(d["s"]["row0"]) + (f if frow else sidx)
            j = int(d["s"]["col0"]) + (sidx if frow else f)
            byte = int(d["dst2"]) - CT_AT
            assert byte >= 0
            e0 = byte if tq in (E4M3, sr.E5M2) else byte * 2 if tq == FP4 else byte * 4 // 3
            assert sr.byte_offset(tq, e0) == byte
            ld = int(d["ldd2"])
            at = e0 + (f * ld + sidx if int(d["flags2"]) & TR else sidx * ld + f)
            assert at.max() < held[r].size
            assert (held[r][at] == ids[j, i]).all(), f"rank {r}: twin of rows {d['s']['row0']}.. cols {d['s']['col0']}.."
            seen[j, i] += 1
    assert n_ops > 0 and (seen == 1).all(), "the twins of all ranks must cover Ct exactly once"


def _custom32(P, grid):
    a_case, c_case = mc.geometry("custom32", "N", grid)
    return a_case, c_case


def test_twin_rule_refused(costa):
    grid, P = (2, 2), 4
    a_case, c_case = _custom32(P, grid)
    m, n = c_case.shape()
    good = dc.twin(c_case, "C")
    # un-transposed owners: some tile's twin lives on another rank
    bad_owners = Custom(list(c_case.colsplit), list(c_case.rowsplit), c_case.owners.copy(), ord="C")
    assert (bad_owners.owners != good.owners).any()
    hit = 0
    for r in range(P):
        A, C, Ct = _layouts(costa, E4M3, a_case, c_case, bad_owners, r, P)
        try:
            costa.plan_export_dual(A, C, Ct, r, P, "N")
        except costa.CostaError as e:
            assert e.code == 1 and "dual layouts" in str(e) and "rows" in str(e), str(e)
            hit += 1
    assert hit > 0
    # finer blocks than the tiles, and a Ct of C's own shape
    a1, c1 = mc.geometry("g192", "N")
    for ct_case in (BC(160, 192, 16, 16), BC(192, 160, 32, 96)):
        A, C, Ct = _layouts(costa, E4M3, a1, c1, ct_case, 0, 1)
        with pytest.raises(costa.CostaError, match="dual layouts") as ei:
            costa.plan_export_dual(A, C, Ct, 0, 1, "N")
        assert ei.value.code == 1
    # coarser blocks are fine
    A, C, Ct = _layouts(costa, E4M3, a1, c1, BC(160, 192, 160, 192), 0, 1)
    assert costa.plan_export_dual(A, C, Ct, 0, 1, "N", c_axis="rows", ct_axis="cols").local_dual.size > 0


def test_block_rule_refused_per_output(costa):
    a_case, c_case = mc.geometry("bc203", "N")  # C in 40 x 24 blocks
    A, C, Ct = _layouts(costa, E4M3, a_case, c_case, dc.twin(c_case, "C"), 0, 1)
    assert costa.plan_export_dual(A, C, Ct, 0, 1, "N").local_dual.size > 0  # the twins exist
    for kw, which in ((dict(c_axis="rows"), "of C:"), (dict(c_axis="cols"), "of C:"), (dict(ct_axis="rows"), "of Ct"),
                      (dict(ct_axis="cols"), "of Ct")):
        with pytest.raises(costa.CostaError, match="MX block") as ei:
            costa.plan_export_dual(A, C, Ct, 0, 1, "N", **kw)
        assert ei.value.code == 1 and which in str(ei.value), str(ei.value)


def test_packed_rules_on_the_ct_side(costa):
    # FP4: an odd leading dimension of Ct
    a_case, c_case = dc.geometry(FP4, "custom32", "N")
    ct = dc.twin(c_case, "C")
    ct.ld_pad = 1
    per, _ = ct._blocks(1)
    assert all(ld % 2 == 1 for _, _, _, ld in per[0])
    blocks = [(CT_AT + off // 2, ld, i, j) for i, j, off, ld in per[0]]
    lay = sr.family(FP4)[2]
    A, C = lay(costa, a_case, 0, A_AT, 1, F), lay(costa, c_case, 0, C_AT, 1, FP4)
    with pytest.raises(costa.CostaError, match="FP4 pair") as ei:
        Ct = costa.custom_layout(*ct.owners.shape, ct.rowsplit, ct.colsplit, ct.owners, blocks, "C", FP4)
        costa.plan_export_dual(A, C, Ct, 0, 1, "N")
    assert ei.value.code == 1
    # FP6: a split point of C's columns off the grid of 4 is a split of Ct's packed dimension
    rs, cs = [0, 64, 128], [0, 34, 68]
    a6 = Custom(rs, cs, [[0, 0], [0, 0]], ord="C")
    c6 = Custom(rs, cs, [[0, 0], [0, 0]], ord="C")
    ct6 = Custom([0, 68], [0, 128], [[0]], ord="C")
    lay = sr.family(E2M3)[2]
    A, C, Ct = lay(costa, a6, 0, A_AT, 1, F), lay(costa, c6, 0, C_AT, 1, E2M3), lay(costa, ct6, 0, CT_AT, 1, E2M3)
    assert costa.plan_export_scaled(A, C, 0, 1, "N", 1.0, 0.0).local_scaled.size == 4  # (A, C) alone is fine
    with pytest.raises(costa.CostaError, match="FP6 quad") as ei:
        costa.plan_export_dual(A, C, Ct, 0, 1, "N")
    assert ei.value.code == 1


def test_other_types_are_refused(costa):
    a_case, c_case = mc.geometry("g192", "N")
    ct_case = dc.twin(c_case, "C")
    lay = sr.family(E4M3)[2]
    A8 = lay(costa, a_case, 0, A_AT, 1, E4M3)
    A, C, Ct = _layouts(costa, E4M3, a_case, c_case, ct_case, 0, 1)
    Ct5 = lay(costa, ct_case, 0, CT_AT, 1, sr.E5M2)
    Cf = lay(costa, c_case, 0, C_AT, 1, F)
    with pytest.raises(costa.CostaError, match="must be COSTA_FLOAT"):
        costa.plan_export_dual(A8, C, Ct, 0, 1, "N")
    for c, ct in ((C, Ct5), (Cf, Ct)):
        with pytest.raises(costa.CostaError, match="no dual MX transform") as ei:
            costa.plan_export_dual(A, c, ct, 0, 1, "N")
        assert "FP8_E4M3" in str(ei.value)
