"""Shared by the MX tests (test_mx_plan_cpu.py, test_gpu_mx.py, mx_loopback_child.py): the numpy /
torch-CPU model of costa_hip.h, "MX block-scaled transforms", on the GLOBAL matrix.

  1. every rank's A buffer is widened and gathered into A's dense matrix (oracle.transform: an exact
     redistribution), multiplied by pow2(SA) expanded to one factor per element (numpy fp32: one
     rounded product, subnormals kept), and turned round for 'T';
  2. v = alpha*x (+ beta*c_old, C gathered the same way) in numpy fp32, products and sum rounded
     separately; alpha = beta = 0 gives zeros;
  3. with c_scales: per block of 32 along the axis the unsigned maximum of the bit patterns of |v|,
     E by the floor (or ceil) rule, q = torch.clamp(v * pow2(254 - E), -fmax, fmax).to(float8 dtype),
     a block with an inf or NaN all NaN with E = 255;
  4. the dense result is placed into every rank's C buffer over its old bytes (padding and gaps keep
     their fill).
Scale bytes are always compared exactly.  Buffers of FP8 are numpy uint8 arrays of raw bits.
"""
import numpy as np

import fp8_common as fc
import oracle
from casegen import Custom
from fp8_common import E4M3, E5M2, F, NAMES, assert_bits, cvt, make_layout, widen  # noqa: F401

ROWS, COLS = 0, 1
FLOOR, CEIL = 0, 1
EMAX = {E4M3: 8, E5M2: 15}
FMAX = {E4M3: np.float32(448.0), E5M2: np.float32(57344.0)}
F_ROWS = 0x80
TRANSPOSE = 0x1


def pow2(E):
    """fp32 of scale bytes: bits E << 23, 0 -> 2^-127 (subnormal), 255 -> NaN"""
    E = np.asarray(E, np.uint32)
    bits = np.where(E == 0, np.uint32(0x00400000), np.where(E == 255, np.uint32(0x7FC00000), E << np.uint32(23)))
    return bits.astype(np.uint32).view(np.float32)


def n_blocks(n):
    return (n + 31) // 32


def expand(S, axis, rows, cols):
    """one pow2 factor per element of a rows x cols matrix from S[block, line]"""
    S = np.asarray(S, np.uint8)
    if axis == ROWS:
        assert S.shape == (n_blocks(rows), cols), S.shape
        return pow2(np.repeat(S, 32, axis=0)[:rows, :])
    assert S.shape == (n_blocks(cols), rows), S.shape
    return pow2(np.repeat(S.T, 32, axis=1)[:, :cols])


def quantise_dense(V, axis, tq, rounding=FLOOR):
    """(q bits m x n uint8, E bytes [block, line], t = the scaled values before the clamp)"""
    import torch
    V = np.ascontiguousarray(V, np.float32)
    W = V if axis == ROWS else V.T          # blocks along W's rows
    along, lines = W.shape
    nb = n_blocks(along)
    pad = np.zeros((nb * 32, lines), np.float32)
    pad[:along] = W
    bits = pad.view(np.uint32) & np.uint32(0x7FFFFFFF)
    amax = bits.reshape(nb, 32, lines).max(axis=1)                 # unsigned maximum of |v| bits
    e = (amax >> np.uint32(23)).astype(np.int64)
    E = np.where(e == 255, 255, np.clip(e - EMAX[tq], 0, 254))
    with np.errstate(all="ignore"):
        if rounding == CEIL:
            over = amax.view(np.float32) * pow2(np.where(E == 255, 0, 254 - E)) > FMAX[tq]
            E = np.where((E != 255) & over & (E < 254), E + 1, E)
        inv = pow2(np.where(E == 255, 255, 254 - E))               # (NaN where E = 255)
        t = pad * np.repeat(inv, 32, axis=0)
        assert t.dtype == np.float32
    t = np.where(np.repeat(E == 255, 32, axis=0), np.float32(np.nan), t)[:along]
    fm = float(FMAX[tq])
    q = torch.clamp(torch.from_numpy(np.ascontiguousarray(t)), -fm, fm).to(fc._torch_dt(tq)).view(torch.uint8).numpy()
    if axis == COLS:
        q, t = q.T, t.T
    return np.ascontiguousarray(q), E.astype(np.uint8), np.ascontiguousarray(t)


def scale_g(x, c_old, alpha, beta):
    """the ordinary ZERO / ALPHA / AXPBY branches in fp32 (1 * x has x's bits for every non-NaN x)"""
    a, b = np.float32(alpha), np.float32(beta)
    with np.errstate(all="ignore"):
        if a == 0 and b == 0:
            return np.zeros_like(x)
        if b == 0:
            return a * x
        return b * c_old + a * x


# ------------------------------------------------------------------ dense <-> layouts
def _dense_case(m, n):
    return Custom([0, m], [0, n], [[0]], ord="C")


def gather(case, P, bufs):
    """dense fp32 matrix of per-rank fp32 buffers"""
    m, n = case.shape()
    out = [np.zeros(m * n, np.float32)] + [np.zeros(1, np.float32) for _ in range(P - 1)]
    oracle.transform(oracle.FLOAT, "N", 1, 0, case.geom(P), [np.ascontiguousarray(b, np.float32) for b in bufs],
                     _dense_case(m, n).geom(P), out)
    return out[0].reshape(n, m).T.copy()


def place(case, P, dense, fill):
    """per-rank fp32 buffers: `fill` with the dense matrix written over its elements"""
    m, n = case.shape()
    src = [np.asfortranarray(dense, np.float32).reshape(-1, order="F").copy()]
    src += [np.zeros(1, np.float32) for _ in range(P - 1)]
    out = [np.ascontiguousarray(f, np.float32).copy() for f in fill]
    oracle.transform(oracle.FLOAT, "N", 1, 0, _dense_case(m, n).geom(P), src, case.geom(P), out)
    return out


def owned(case, P, rank):
    """dense bool matrix: the elements of the matrix that live on `rank`"""
    bufs = [np.full(case.buf_elems(r, P), 1.0 if r == rank else 0.0, np.float32) for r in range(P)]
    return gather(case, P, bufs) == 1.0


def scale_bytes(seed, shape, lo=120, hi=134):
    """input scale bytes around 127"""
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def quant_data(seed, n, tq=None):
    """n fp32 values: uniform +-1 times 2^k, k per run of 32 elements in -6 .. 6, so that blocks have
    different exponents and about one element in eight exceeds fmax before the clamp under FLOOR"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    k = np.repeat(rng.integers(-6, 7, (n + 31) // 32), 32)[:n]
    return (v * np.exp2(k).astype(np.float32)).astype(np.float32)


def expected_transform_mx(ta, tc, op, alpha, beta, a_case, c_case, P, a_bufs, c_bufs, sa=None, a_axis=ROWS,
                          c_axis=None, rounding=FLOOR):
    """-> (expected C buffer of every rank in tc, SC[block, line] or None, t before the clamp or None)"""
    am, an = a_case.shape()
    X = gather(a_case, P, [widen(a, ta) for a in a_bufs])
    if sa is not None:
        with np.errstate(all="ignore"):
            X = X * expand(sa, a_axis, am, an)
    if op != "N":
        X = X.T
    wc = [widen(c, tc) for c in c_bufs]
    V = scale_g(np.ascontiguousarray(X, np.float32), gather(c_case, P, wc) if beta != 0 else None, alpha, beta)
    assert V.dtype == np.float32 and V.shape == tuple(c_case.shape())
    if c_axis is None:
        assert tc == F
        return place(c_case, P, V, wc), None, None
    q, E, t = quantise_dense(V, c_axis, tc, rounding)
    out = place(c_case, P, widen(q.reshape(-1), tc).reshape(q.shape), wc)
    return [cvt(o, tc) for o in out], E, t


def assert_data_finite(exp, code, what):
    """no NaN and no inf expected, so assert_bits' "a NaN only asks for a NaN" rule hides nothing"""
    assert np.isfinite(widen(exp, code)).all(), f"{what}: the expected buffer holds a NaN or an inf"


# ------------------------------------------------------------------ the tile-boundary rule
def boundary_ok(sops, axis, m, n):
    """the rule of costa_hip.h on scaled ops, in Python"""
    for t in sops:
        nf, ns, flags = int(t["op"]["nf"]), int(t["op"]["ns"]), int(t["op"]["flags"])
        if nf <= 0 or ns <= 0:
            continue
        frow = bool(flags & F_ROWS)
        at = int(t["row0"]) if axis == ROWS else int(t["col0"])
        ln = nf if (axis == ROWS) == frow else ns
        edge = m if axis == ROWS else n
        if at % 32 or (ln % 32 and at + ln != edge):
            return False
    return True


# ------------------------------------------------------------------ tile lists
def op_index(t):
    """(source element offsets, destination element offsets, target i, target j) of one scaled op
    whose src / dst count ELEMENTS; all nf x ns"""
    nf, ns = int(t["op"]["nf"]), int(t["op"]["ns"])
    flags = int(t["op"]["flags"])
    f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
    si = int(t["op"]["src"]) + s * int(t["op"]["lds"]) + f
    di = int(t["op"]["dst"]) + (f * int(t["op"]["ldd"]) + s if flags & TRANSPOSE else s * int(t["op"]["ldd"]) + f)
    if flags & F_ROWS:
        return si, di, int(t["row0"]) + f, int(t["col0"]) + s
    return si, di, int(t["row0"]) + s, int(t["col0"]) + f


def expected_tiles_mx(ta, tc, sops, alpha, beta, a, c, m, n, sa=None, a_axis=ROWS, a_transposed=False,
                      c_axis=None, rounding=FLOOR, sc_fill=None):
    """-> (expected destination buffer in tc, expected c_scales tensor [block, line] over sc_fill,
    t before the clamp on the covered elements).  The ops' target regions are disjoint."""
    wa, wc = widen(a, ta), widen(c, tc)
    V = np.zeros((m, n), np.float32)
    cov = np.zeros((m, n), bool)
    fac = None
    if sa is not None:
        fac = expand(sa, a_axis, n, m).T if a_transposed else expand(sa, a_axis, m, n)
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
    if c_axis is None:
        for t in sops:
            si, di, i, j = op_index(t)
            out[di] = V[i, j]
        return out, None, None
    q, E, tt = quantise_dense(V, c_axis, tc, rounding)
    ob = np.ascontiguousarray(c, np.uint8).copy()
    for t in sops:
        si, di, i, j = op_index(t)
        ob[di] = q[i, j]
    # a block is written when an op covers its first element
    Wc = cov if c_axis == ROWS else cov.T
    first = Wc[::32, :]
    sc = np.asarray(sc_fill, np.uint8).copy()
    assert sc.shape == E.shape
    sc[first] = E[first]
    return ob, sc, np.where(cov, tt, 0)


# ------------------------------------------------------------------ geometries
def geometry(name, op, grid=(1, 1)):
    """(A case, C case): the accepted geometries of the tile-boundary rule (block sizes and split
    points multiples of 32; partial last blocks at the matrix edge), or one of half_common.geometry
    (bc203, cfg5: not aligned, dequantise only)"""
    from casegen import BC
    import half_common
    t = op != "N"
    pm, pn = grid
    P = pm * pn
    kw = dict(pm=pm, pn=pn)

    def dims(m, n):
        return (n, m) if t else (m, n)
    if name == "g192":
        return BC(*dims(192, 160), 64, 32, **kw), BC(192, 160, 32, 96, **kw)
    if name == "g203":
        return BC(*dims(203, 157), 64, 96, **kw), BC(203, 157, 96, 32, **kw)
    if name == "g203pad":
        return BC(*dims(203, 157), 64, 96, lld_pad=1, **kw), BC(203, 157, 96, 32, lld_pad=1, **kw)
    if name == "custom32":
        rs, cs = [0, 64, 96, 200], [0, 32, 128, 170]
        ars, acs = [0, 96, 200], [0, 64, 170]
        if t:
            ars, acs = acs, ars

        def owners(nr, nc, k):
            i, j = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
            return ((i * k + j) % P).astype(np.int32)
        return (Custom(ars, acs, owners(len(ars) - 1, len(acs) - 1, 1), ord="R", ld_pad=1, gap=3),
                Custom(rs, cs, owners(len(rs) - 1, len(cs) - 1, 3), ord="C", ld_pad=2, gap=5))
    return half_common.geometry(name, op, grid)
