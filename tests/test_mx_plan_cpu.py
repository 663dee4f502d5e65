"""MX block-scaled transforms without a GPU: the tile-boundary rule on exported scaled plans
(costa_hip_mx_check_ops against the rule written out in mx_common.boundary_ok), the stride / aliasing
rule of the descriptors, and the model's own arithmetic on hand-made blocks."""
import numpy as np
import pytest

import mx_common as mc
from mx_common import COLS, E4M3, E5M2, F, ROWS

GRIDS = {"1x1": (1, 1), "2x2": (2, 2)}


def _plan_ops(costa, geom, op, grid, ta=F, tc=E4M3):
    pm, pn = GRIDS[grid]
    P = pm * pn
    a_case, c_case = mc.geometry(geom, op, (pm, pn))
    out = []
    for r in range(P):
        A = mc.make_layout(costa, a_case, r, 1 << 40, P, ta)
        C = mc.make_layout(costa, c_case, r, 1 << 41, P, tc)
        s = costa.plan_export_scaled(A, C, r, P, op, 1.0, 0.0)
        out += [s.local_scaled, s.unpack_scaled]
    return c_case.shape(), out


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("geom", ["g192", "g203", "g203pad", "custom32"])
def test_rule_accepts_layouts_on_multiples_of_32(costa, geom, op, grid):
    (m, n), lists = _plan_ops(costa, geom, op, grid)
    assert sum(x.size for x in lists) > 0
    for axis in (ROWS, COLS):
        for ops in lists:
            assert mc.boundary_ok(ops, axis, m, n)
            costa.mx_check_ops(ops, axis, m, n)
    if geom in ("g203", "g203pad"):  # partial last blocks at the matrix edge take part
        assert any((ops["row0"] + np.where(ops["op"]["flags"] & mc.F_ROWS, ops["op"]["nf"], ops["op"]["ns"]) == 203).any()
                   for ops in lists)


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("axis", [ROWS, COLS])
def test_rule_refuses_40_by_24_blocks(costa, op, grid, axis):
    (m, n), lists = _plan_ops(costa, "bc203", op, grid)
    assert not all(mc.boundary_ok(ops, axis, m, n) for ops in lists)
    with pytest.raises(costa.CostaError, match="MX block") as ei:
        for ops in lists:
            costa.mx_check_ops(ops, axis, m, n)
    assert ei.value.code == 1


def test_rule_on_single_ops(costa):
    def one(row0, col0, nf, ns, frow=True):
        t = np.zeros(1, costa.SCALED_OP_DTYPE)
        t["op"]["nf"], t["op"]["ns"], t["op"]["lds"], t["op"]["ldd"] = nf, ns, nf, nf
        t["op"]["flags"] = mc.F_ROWS if frow else 0
        t["row0"], t["col0"] = row0, col0
        return t
    m, n = 109, 77
    costa.mx_check_ops(one(64, 5, 32, 7), ROWS, m, n)
    costa.mx_check_ops(one(64, 5, 45, 7), ROWS, m, n)           # ends at the edge: a partial block of 13
    costa.mx_check_ops(one(3, 64, 9, 13), COLS, m, n)           # 13 columns up to the edge
    costa.mx_check_ops(one(5, 32, 32, 9, frow=False), COLS, m, n)
    for bad, axis in ((one(64, 5, 44, 7), ROWS), (one(16, 0, 32, 7), ROWS), (one(0, 8, 9, 32), COLS),
                      (one(5, 32, 31, 9, frow=False), COLS)):
        assert not mc.boundary_ok(bad, axis, m, n)
        with pytest.raises(costa.CostaError, match="MX block"):
            costa.mx_check_ops(bad, axis, m, n)


def test_strides_and_aliasing(costa):
    rows, cols = 203, 157                     # ROWS: 7 blocks x 157 lines; COLS: 5 blocks x 203 lines
    ok = [(ROWS, 157, 1), (ROWS, 1, 7), (ROWS, 1, 9), (ROWS, 200, 1), (COLS, 203, 1), (COLS, 1, 5), (ROWS, 2, 14),
          (ROWS, 3, 7)]                       # (3, 7): db = 7 would be needed, only 0 .. 6 exist
    bad = [(ROWS, 0, 1), (ROWS, 1, 0), (ROWS, -157, 1), (ROWS, 1, -7), (ROWS, 1, 1), (ROWS, 1, 6), (ROWS, 156, 1),
           (COLS, 1, 4), (COLS, 202, 1), (ROWS, 2, 3), (ROWS, 6, 4)]
    for axis, bs, ls in ok:
        costa.mx_check_scales(costa.MxScales(0, axis, bs, ls), rows, cols)
        assert _distinct(axis, bs, ls, rows, cols), (axis, bs, ls)
    for axis, bs, ls in bad:
        assert bs <= 0 or ls <= 0 or not _distinct(axis, bs, ls, rows, cols), (axis, bs, ls)
        with pytest.raises(costa.CostaError) as ei:
            costa.mx_check_scales(costa.MxScales(0, axis, bs, ls), rows, cols)
        assert ei.value.code == 1, (axis, bs, ls)
    with pytest.raises(costa.CostaError):
        costa.mx_check_scales(costa.MxScales(0, 2, 1, 7), rows, cols)


def _distinct(axis, bs, ls, rows, cols):
    nb, lines = ((rows + 31) // 32, cols) if axis == ROWS else ((cols + 31) // 32, rows)
    at = np.arange(nb)[:, None] * bs + np.arange(lines)[None, :] * ls
    return np.unique(at).size == at.size


@pytest.mark.parametrize("tq", [E4M3, E5M2])
def test_model_on_hand_made_blocks(tq):
    """the model itself: E of known maxima, the clamp under FLOOR, no saturation under CEIL, specials"""
    emax, fmax = mc.EMAX[tq], float(mc.FMAX[tq])
    V = np.zeros((32, 8), np.float32)
    V[3, 0] = 1.0                               # amax 2^0: E = 127 - emax, q = 2^emax
    V[5, 1] = fmax * 2.0 ** -3                  # amax = fmax * 2^-3: scaled exactly onto fmax
    V[7, 2] = 1.9375                            # scales into (fmax, 2^(emax+1)): clamps under FLOOR
    V[:, 3] = np.float32(1e-42)                 # all subnormal: E = 0
    V[9, 4] = np.nan
    V[9, 5] = np.inf
    V[2, 6] = -0.0
    q, E, t = mc.quantise_dense(V, ROWS, tq, mc.FLOOR)
    assert E.shape == (1, 8)
    assert list(E[0, :4]) == [127 - emax, 127 - 3, 127 - emax, 0]
    w = mc.widen(q.reshape(-1), tq).reshape(32, 8)
    assert w[3, 0] == 2.0 ** emax and w[5, 1] == fmax and w[7, 2] == fmax and t[7, 2] > fmax
    assert E[0, 4] == 255 and E[0, 5] == 255 and np.isnan(w[:, 4]).all() and np.isnan(w[:, 5]).all()
    assert E[0, 6] == 0 and q[2, 6] == 0x80 and (np.delete(q[:, 6], 2) == 0).all() and E[0, 7] == 0
    q2, E2, t2 = mc.quantise_dense(V, ROWS, tq, mc.CEIL)
    assert list(E2[0, :4]) == [127 - emax, 127 - 3, 127 - emax + 1, 0]
    assert (np.abs(t2[:, :4]) <= fmax).all()
    # the same blocks along columns
    q3, E3, _ = mc.quantise_dense(V.T.copy(), COLS, tq, mc.FLOOR)
    assert (q3 == q.T).all() and (E3 == E).all()
    # pow2 of the special bytes
    p = mc.pow2(np.array([0, 1, 127, 254, 255], np.uint8)).view(np.uint32)
    assert list(p) == [0x00400000, 0x00800000, 0x3F800000, 0x7F000000, 0x7FC00000]
