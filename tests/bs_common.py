"""Shared by the block-scaled FP8 tests (test_bs_model_cpu.py, test_bs_plan_cpu.py, test_gpu_bs.py,
bs_loopback_child.py): the numpy / torch-CPU model of costa_hip.h, "Block-scaled FP8 transforms (fp32
scales)", on the GLOBAL matrix, written from the semantics alone.

  1. every rank's A buffer is widened and gathered into A's dense matrix, multiplied by SA expanded to
     one factor per element (numpy fp32: one rounded product), and turned round for 'T';
  2. v = alpha*x (+ beta*c_old) in numpy fp32 (mx_common.scale_g);
  3. with c_scales: per block the unsigned maximum of the bit patterns of |v|; exponent 255 -> S = NaN
     and the block all NaN; else amax_c = max(amax, 2^-40), EXACT: S = amax_c / fmax, R = fmax / amax_c
     (numpy fp32 divisions), POW2: E by the MX ceil rule on amax_c, S = 2^(E-127), R = 2^(127-E);
     q = torch.clamp(v * R, -fmax, fmax).to(float8 dtype);
  4. the dense result is placed into every rank's C buffer over its old bytes.
Scale floats are compared by their bits.  Buffers of FP8 are numpy uint8 arrays of raw bits.
"""
import numpy as np

import fp8_common as fc
from casegen import BC, Custom
from fp8_common import E4M3, E5M2, F, NAMES, assert_bits, cvt, make_layout, widen  # noqa: F401
from mx_common import (EMAX, F_ROWS, FMAX, TRANSPOSE, gather, op_index, owned, place, quant_data,  # noqa: F401
                       scale_g)

EXACT, POW2 = 0, 1
RND = {EXACT: "exact", POW2: "pow2"}
SHAPES = [(1, 128), (128, 1), (128, 128)]
SHAPE_IDS = ["1x128", "128x1", "128x128"]
EPS_BITS = np.uint32(0x2B800000)  # 2^-40
NAN_BITS = np.uint32(0x7FC00000)


def n_blocks(shape, block):
    return (-(-shape[0] // block[0]), -(-shape[1] // block[1]))


def expand(S, block, rows, cols):
    """one factor per element of a rows x cols matrix from S[block row, block column]"""
    S = np.asarray(S, np.float32)
    assert S.shape == n_blocks((rows, cols), block), (S.shape, block, rows, cols)
    return np.repeat(np.repeat(S, block[0], axis=0), block[1], axis=1)[:rows, :cols]


def block_amax_bits(V, block):
    """[block row, block column] unsigned maxima of the bits of |v| (absent elements count as 0)"""
    m, n = V.shape
    nbr, nbc = n_blocks((m, n), block)
    pad = np.zeros((nbr * block[0], nbc * block[1]), np.uint32)
    pad[:m, :n] = np.ascontiguousarray(V, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return pad.reshape(nbr, block[0], nbc, block[1]).max(axis=(1, 3))


def scales_of(amax_bits, tq, rounding):
    """(S, R) fp32 arrays of the blocks' amax bit patterns"""
    amax_bits = np.asarray(amax_bits, np.uint32)
    special = (amax_bits >> np.uint32(23)) == 255
    ac = np.maximum(amax_bits, EPS_BITS)
    ac = np.where(special, EPS_BITS, ac).astype(np.uint32).view(np.float32)
    fm = FMAX[tq]
    with np.errstate(all="ignore"):
        if rounding == EXACT:
            S, R = ac / fm, fm / ac
        else:
            e = (ac.view(np.uint32) >> np.uint32(23)).astype(np.int64)
            E = np.clip(e - EMAX[tq], 0, 254)
            over = ac * ((254 - E).astype(np.uint32) << np.uint32(23)).view(np.float32) > fm
            E = np.where(over & (E < 254), E + 1, E)
            assert ((E >= 1) & (E <= 253)).all()
            S = (E.astype(np.uint32) << np.uint32(23)).view(np.float32)
            R = ((254 - E).astype(np.uint32) << np.uint32(23)).view(np.float32)
    assert S.dtype == np.float32 and R.dtype == np.float32
    S = np.where(special, NAN_BITS, S.view(np.uint32)).astype(np.uint32).view(np.float32)
    R = np.where(special, NAN_BITS, R.view(np.uint32)).astype(np.uint32).view(np.float32)
    return S, R


def quantise_dense(V, block, tq, rounding=EXACT):
    """(q bits m x n uint8, S [block row, block column] fp32, t = the scaled values before the clamp)"""
    import torch
    V = np.ascontiguousarray(V, np.float32)
    m, n = V.shape
    S, R = scales_of(block_amax_bits(V, block), tq, rounding)
    with np.errstate(all="ignore"):
        t = V * expand(R, block, m, n)
    assert t.dtype == np.float32
    fm = float(FMAX[tq])
    q = torch.clamp(torch.from_numpy(np.ascontiguousarray(t)), -fm, fm).to(fc._torch_dt(tq)).view(torch.uint8).numpy()
    return np.ascontiguousarray(q), S, t


def special_matrix():
    """one 128 x 1 block per column"""
    V = np.zeros((128, 8), np.float32)
    V[:, 1] = np.float32(2.0 ** -45) * np.linspace(-1, 1, 128, dtype=np.float32)   # amax below 2^-40
    V[:, 2] = np.float32(1e-42) * np.arange(1, 129, dtype=np.float32)              # all subnormal
    V[:, 3] = 0.25
    V[9, 3] = np.nan
    V[:, 4] = -0.5
    V[77, 4] = -np.inf
    V[2, 5] = -0.0
    V[:, 6] = np.float32(2.5e38) * np.linspace(-1, 1, 128, dtype=np.float32)
    V[:, 7] = np.float32(2.0 ** -126)
    return V


def scale_floats(seed, shape):
    """input scales: positive, a few binades around 2^-6, not powers of two"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(-9, -3, shape))).astype(np.float32)


def assert_float_bits(got, exp, what):
    g, e = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(exp, np.float32).view(np.uint32)
    assert g.shape == e.shape, f"{what}: shape {g.shape}, expected {e.shape}"
    bad = np.flatnonzero(g.reshape(-1) != e.reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {e.size} scale floats differ, first at {bad[0]}: got "
                           f"{int(g.reshape(-1)[bad[0]]):#x}, expected {int(e.reshape(-1)[bad[0]]):#x}")


def expected_transform_bs(ta, tc, op, alpha, beta, a_case, c_case, P, a_bufs, c_bufs, sa=None, a_block=None,
                          c_block=None, rounding=EXACT):
    """-> (expected C buffer of every rank in tc, SC[block row, block column] or None, t or None)"""
    am, an = a_case.shape()
    X = gather(a_case, P, [widen(a, ta) for a in a_bufs])
    if sa is not None:
        with np.errstate(all="ignore"):
            X = X * expand(sa, a_block, am, an)
    if op != "N":
        X = X.T
    wc = [widen(c, tc) for c in c_bufs]
    V = scale_g(np.ascontiguousarray(X, np.float32), gather(c_case, P, wc) if beta != 0 else None, alpha, beta)
    assert V.dtype == np.float32 and V.shape == tuple(c_case.shape())
    if c_block is None:
        assert tc == F
        return place(c_case, P, V, wc), None, None
    q, S, t = quantise_dense(V, c_block, tc, rounding)
    out = place(c_case, P, widen(q.reshape(-1), tc).reshape(q.shape), wc)
    return [cvt(o, tc) for o in out], S, t


def expected_tiles_bs(ta, tc, sops, alpha, beta, a, c, m, n, sa=None, a_block=None, a_transposed=False,
                      c_block=None, rounding=EXACT, sc_fill=None):
    """-> (expected destination buffer in tc, expected c_scales tensor over sc_fill, t on the covered
    elements).  The ops' target regions are disjoint and, with c_block, cover whole blocks of the m x n
    matrix."""
    wa, wc = widen(a, ta), widen(c, tc)
    V = np.zeros((m, n), np.float32)
    cov = np.zeros((m, n), bool)
    fac = None
    if sa is not None:
        fac = expand(sa, a_block, n, m).T if a_transposed else expand(sa, a_block, m, n)
    for t in sops:
        si, di, i, j = op_index(t)
        assert not cov[i, j].any(), "ops overlap in target coordinates"
        cov[i, j] = True
        x = wa[si]
        with np.errstate(all="ignore"):
            if fac is not None:
                x = x * fac[i, j]
        V[i, j] = scale_g(x.astype(np.float32), wc[di], alpha, beta)
    out = wc.copy()
    if c_block is None:
        for t in sops:
            si, di, i, j = op_index(t)
            out[di] = V[i, j]
        return out, None, None
    q, S, tt = quantise_dense(V, c_block, tc, rounding)
    ob = np.ascontiguousarray(c, np.uint8).copy()
    for t in sops:
        si, di, i, j = op_index(t)
        ob[di] = q[i, j]
    first = cov[::c_block[0], ::c_block[1]]  # a block is written when an op covers its first element
    sc = np.asarray(sc_fill, np.float32).copy()
    assert sc.shape == S.shape
    sc[first] = S[first]
    return ob, sc, np.where(cov, tt, 0)


# ------------------------------------------------------------------ the tile-boundary rule
def boundary_ok(sops, block, m, n):
    """the rule of costa_hip.h on scaled ops, in Python"""
    for t in sops:
        nf, ns, flags = int(t["op"]["nf"]), int(t["op"]["ns"]), int(t["op"]["flags"])
        if nf <= 0 or ns <= 0:
            continue
        frow = bool(flags & F_ROWS)
        for at, ln, b, edge in ((int(t["row0"]), nf if frow else ns, block[0], m),
                                (int(t["col0"]), ns if frow else nf, block[1], n)):
            if at % b or (ln % b and at + ln != edge):
                return False
    return True


# ------------------------------------------------------------------ geometries
M, N = 330, 270  # 2 * 128 + 74, 2 * 128 + 14: interior, edge and corner blocks


def geometry(name, op, grid=(1, 1)):
    """(A case, C case) of the 330 x 270 matrix: split points on multiples of 128, or `bc203`
    (half_common.geometry: off the grid, dequantise only)"""
    import half_common
    t = op != "N"
    pm, pn = grid
    P = pm * pn
    kw = dict(pm=pm, pn=pn)

    def dims(m, n):
        return (n, m) if t else (m, n)
    if name == "bc128":
        return BC(*dims(M, N), 128, 128, **kw), BC(M, N, 256, 128, **kw)
    if name == "bc128pad":
        return BC(*dims(M, N), 128, 128, lld_pad=1, **kw), BC(M, N, 256, 128, lld_pad=1, **kw)
    if name == "custom128":
        rs, cs = [0, 128, 330], [0, 256, 270]
        ars, acs = [0, 256, 330], [0, 128, 256, 270]
        if t:
            ars, acs = acs, ars

        def owners(nr, nc, k):
            i, j = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
            return ((i * k + j) % P).astype(np.int32)
        return (Custom(ars, acs, owners(len(ars) - 1, len(acs) - 1, 1), ord="R", ld_pad=1, gap=3),
                Custom(rs, cs, owners(len(rs) - 1, len(cs) - 1, 3), ord="C", ld_pad=2, gap=5))
    return half_common.geometry(name, op, grid)
