"""Shared by the stochastic-rounding tests (test_mx_sr_model_cpu.py, test_gpu_mx_sr.py,
mx_sr_loopback_child.py): the numpy model of costa_hip.h, "Stochastic rounding in the MX transforms".

  fmix32, keys, rand24(seed, i, j)   the 24 random bits of target element (i, j), uint32 arithmetic
  mags(type)                         the finite magnitudes of a type in code order, built from the
                                     existing widen of every code (fp8_common, fp4_common, fp6_common)
  sr_codes(t, U, type)               the conversion in float64 from that table: lo / hi search, T =
                                     floor((a - lo) / (hi - lo) * 2^24) (exact: every step of these types
                                     is a power of two), up when T + U >= 2^24; independent of the
                                     kernel's integer routine
  rn_codes(t, type)                  the round-to-nearest codes of the existing models
expected_transform_mx_sr / expected_tiles_mx_sr take E and the pre-clamp t from the existing model
functions (mx_common / fp4_common / fp6_common by the type), clamp, apply sr_codes at the GLOBAL (i, j) of
C's matrix and place the codes as those functions do.  Codes are one uint8 per element, unpacked.
"""
from types import SimpleNamespace

import numpy as np

import fp4_common as f4
import fp6_common as f6
import mx_common as mc
from mx_common import CEIL, COLS, E4M3, E5M2, F, FLOOR, ROWS  # noqa: F401

FP4 = f4.FP4
E2M3, E3M2 = f6.E2M3, f6.E3M2
QTYPES = (E4M3, E5M2, FP4, E2M3, E3M2)
NAMES = {F: "f32", E4M3: "e4m3", E5M2: "e5m2", FP4: "e2m1", E2M3: "e2m3", E3M2: "e3m2"}
FMAX = {E4M3: np.float32(448.0), E5M2: np.float32(57344.0), FP4: np.float32(6.0), E2M3: np.float32(7.5),
        E3M2: np.float32(28.0)}
SIGN = {E4M3: 0x80, E5M2: 0x80, FP4: 8, E2M3: 32, E3M2: 32}
SIGN_SHIFT = {E4M3: 24, E5M2: 24, FP4: 28, E2M3: 26, E3M2: 26}   # fp32 bit 31 -> the code's sign bit
NAN_CODE = {E4M3: 0x7F, E5M2: 0x7F, FP4: 0, E2M3: 0, E3M2: 0}     # what a NaN t (a block with E = 255) stores
M24 = 1 << 24


# ------------------------------------------------------------------ the random bits
def fmix32(h):
    h = np.asarray(h, np.uint64) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(16))


def keys(seed):
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    return (int(fmix32((seed & 0xFFFFFFFF) ^ 0x9E3779B9)), int(fmix32((seed >> 32) ^ 0x85EBCA6B)))


def rand24(seed, i, j):
    """U(seed, i, j) for arrays (or scalars) of zero-based rows and columns -> uint32"""
    k0, k1 = keys(seed)
    i = np.asarray(i, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    j = np.asarray(j, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    inner = (fmix32(i ^ np.uint64(k0)) + j) & np.uint64(0xFFFFFFFF)
    return (fmix32(inner ^ np.uint64(k1)) >> np.uint64(8)).astype(np.uint32)


def rand24_grid(seed, m, n, i0=0, j0=0):
    i, j = np.meshgrid(np.arange(i0, i0 + m, dtype=np.int64), np.arange(j0, j0 + n, dtype=np.int64), indexing="ij")
    return rand24(seed, i, j)


# ------------------------------------------------------------------ the types
def widen_codes(codes, tq):
    """fp32 of unpacked codes, by the existing widen of the type"""
    c = np.ascontiguousarray(codes, np.uint8)
    if tq in (E4M3, E5M2):
        return mc.widen(c.reshape(-1), tq).reshape(c.shape)
    if tq == FP4:
        return f4.w4(c)
    return f6.w6(c, tq)


_MAGS = {}


def mags(tq):
    """float64 magnitudes m_0 = 0 < .. < m_K = fmax of the non-negative finite codes 0 .. K"""
    if tq not in _MAGS:
        n = {E4M3: 0x7F, E5M2: 0x7C, FP4: 8, E2M3: 32, E3M2: 32}[tq]
        m = widen_codes(np.arange(n, dtype=np.uint8), tq).astype(np.float64)
        assert np.isfinite(m).all() and m[0] == 0 and (np.diff(m) > 0).all() and m[-1] == float(FMAX[tq])
        _MAGS[tq] = m
    return _MAGS[tq]


def sr_parts(t, tq):
    """(k, T, step) per element of a clamped finite t: the code of lo, T = floor(frac * 2^24) (0 where
    |t| is representable) and hi - lo (the last step where |t| = fmax)"""
    m = mags(tq)
    a = np.abs(np.asarray(t, np.float32).astype(np.float64))
    k = np.searchsorted(m, a, side="right") - 1
    assert (k >= 0).all() and (a <= m[-1]).all()
    lo = m[k]
    hi = m[np.minimum(k + 1, m.size - 1)]
    step = np.where(k + 1 < m.size, hi - lo, m[-1] - m[-2])
    T = np.floor((a - lo) / step * M24).astype(np.int64)
    assert ((T >= 0) & (T < M24)).all()
    return k, T, step


def sr_codes(t, U, tq):
    """codes of clamped t (fp32, |t| <= fmax or NaN) under the random bits U"""
    t = np.ascontiguousarray(t, np.float32)
    U = np.broadcast_to(np.asarray(U, np.int64), t.shape)
    assert ((U >= 0) & (U < M24)).all()
    nan = np.isnan(t)
    k, T, _ = sr_parts(np.where(nan, np.float32(0), t), tq)
    code = (k + (T + U >= M24)).astype(np.uint32)
    code |= (t.view(np.uint32) >> np.uint32(SIGN_SHIFT[tq])) & np.uint32(SIGN[tq])
    return np.where(nan, np.uint8(NAN_CODE[tq]), code.astype(np.uint8)).astype(np.uint8)


def rn_codes(t, tq):
    """the round-to-nearest-even codes of the existing models for clamped t"""
    t = np.ascontiguousarray(t, np.float32)
    if tq in (E4M3, E5M2):
        return mc.cvt(t.reshape(-1), tq).reshape(t.shape)
    with np.errstate(invalid="ignore"):
        return f4.cvt4(t) if tq == FP4 else f6.cvt6(t, tq)


def clamp(t, tq):
    with np.errstate(invalid="ignore"):
        return np.clip(np.ascontiguousarray(t, np.float32), -FMAX[tq], FMAX[tq]).astype(np.float32)


# ------------------------------------------------------------------ buffers of a type
def unpack(buf, tq):
    if tq == FP4:
        return f4.unpack(buf)
    if tq in f6.FP6:
        return f6.unpack(buf)
    return np.ascontiguousarray(buf, np.uint8).reshape(-1).copy()


def pack(codes, tq):
    if tq == FP4:
        return f4.pack(codes)
    if tq in f6.FP6:
        return f6.pack(codes)
    return np.ascontiguousarray(codes, np.uint8).reshape(-1).copy()


def widen(buf, code):
    """a buffer of `code` -> fp32 per element"""
    if code == F:
        return np.ascontiguousarray(buf, np.float32).copy()
    return widen_codes(unpack(buf, code), code)


def narrow(x, code):
    """fp32 per element -> a buffer of `code` (exact for values that are the widening of a code)"""
    if code == F:
        return np.ascontiguousarray(x, np.float32).copy()
    return pack(rn_codes(x, code), code)


def family(tq):
    """(expected_transform_mx, expected_tiles_mx, make_layout, fill, assert_same) of the type's model"""
    if tq == FP4:
        return f4.expected_transform_mx4, f4.expected_tiles_mx4, f4.make_layout, f4.fill, f4.assert_same
    if tq in f6.FP6:
        return f6.expected_transform_mx6, f6.expected_tiles_mx6, f6.make_layout, f6.fill, f6.assert_same
    return mc.expected_transform_mx, mc.expected_tiles_mx, mc.make_layout, mc.fc.gen, mc.assert_bits


def buf_bytes(code, n):
    return n * 4 if code == F else n if code in (E4M3, E5M2) else n // 2 if code == FP4 else n * 3 // 4


def byte_offset(code, off):
    """byte offset of element offset `off` in a buffer of `code`"""
    if code == FP4:
        assert (np.asarray(off) % 2 == 0).all()
    if code in f6.FP6:
        assert (np.asarray(off) % 4 == 0).all()
    return off * 4 if code == F else off if code in (E4M3, E5M2) else off // 2 if code == FP4 else off * 3 // 4


def source_data(code, seed, n):
    """the inputs of the existing tests: mx_common.quant_data for fp32, its FP8 conversion, random codes"""
    if code == F:
        return mc.quant_data(seed, n)
    if code in (E4M3, E5M2):
        return mc.cvt(mc.quant_data(seed, n), code)
    return f4.fp4_data(seed, n) if code == FP4 else f6.fp6_data(seed, n)


# ------------------------------------------------------------------ expected values
class Shares:
    """what a comparison must see on the model so that it cannot hide a failure: of the elements whose t
    is not representable at least 20 % round down and at least 20 % up, and the SR codes differ from the
    round-to-nearest codes in at least 10 % of the elements"""

    def __init__(self, t, U, sr, tq, mask=None):
        mask = np.ones(t.shape, bool) if mask is None else mask
        fin = mask & ~np.isnan(t)
        tt = np.where(fin, t, np.float32(0))
        k, T, _ = sr_parts(tt, tq)
        inexact = fin & (T > 0)
        up = (sr & np.uint8(SIGN[tq] - 1)) > k
        self.n, self.inexact = int(mask.sum()), int(inexact.sum())
        self.up = float((up & inexact).sum()) / max(self.inexact, 1)
        self.down = float((~up & inexact).sum()) / max(self.inexact, 1)
        self.differs = float(((sr != rn_codes(tt, tq)) & fin).sum()) / max(self.n, 1)

    def check(self, what):
        assert self.inexact > 0 and self.down >= 0.2 and self.up >= 0.2 and self.differs >= 0.1, \
            f"{what}: down {self.down:.3f}, up {self.up:.3f} of {self.inexact} inexact, differs {self.differs:.3f} of {self.n}"

    def __repr__(self):
        return f"down {self.down:.3f} up {self.up:.3f} of {self.inexact}, differs {self.differs:.3f} of {self.n}"


def expected_transform_mx_sr(seed, ta, tc, op, alpha, beta, a_case, c_case, P, a_bufs, c_bufs, sa=None, a_axis=ROWS,
                             c_axis=ROWS, rounding=FLOOR):
    """-> exp: the expected C buffer of every rank in tc, rn: the same of the call without a seed, sc:
    SC[block, line], t_pre / t: the dense t before / after the clamp, q: the dense SR codes, shares"""
    xf = family(tc)[0]
    rn, E, t_pre = xf(ta, tc, op, alpha, beta, a_case, c_case, P, a_bufs, c_bufs, sa=sa, a_axis=a_axis, c_axis=c_axis,
                  rounding=rounding)
    m, n = c_case.shape()
    t = clamp(t_pre, tc)
    U = rand24_grid(seed, m, n)
    q = sr_codes(t, U, tc)
    wc = [widen(c, tc) for c in c_bufs]
    out = mc.place(c_case, P, widen_codes(q, tc), wc)
    return SimpleNamespace(exp=[narrow(o, tc) for o in out], rn=rn, sc=E, t_pre=t_pre, t=t, q=q,
                           shares=Shares(t, U, q, tc))


def expected_tiles_mx_sr(seed, ta, tc, sops, alpha, beta, a, c, m, n, sa=None, a_axis=ROWS, a_transposed=False,
                         c_axis=ROWS, rounding=FLOOR, sc_fill=None):
    """-> exp: the expected destination buffer in tc, rn: the same of the call without a seed, sc: the
    expected c_scales over sc_fill, t_pre / t: t before / after the clamp on the covered elements (0
    elsewhere), q: the SR codes there, cov: the covered elements, shares over them.  The ops' src / dst
    count ELEMENTS."""
    tiles = family(tc)[1]
    rn, sc, t_pre = tiles(ta, tc, sops, alpha, beta, a, c, m, n, sa=sa, a_axis=a_axis, a_transposed=a_transposed,
                      c_axis=c_axis, rounding=rounding, sc_fill=sc_fill)
    t = clamp(t_pre, tc)
    U = rand24_grid(seed, m, n)
    q = sr_codes(t, U, tc)
    oc = unpack(c, tc)
    cov = np.zeros((m, n), bool)
    for o in sops:
        si, di, i, j = mc.op_index(o)
        oc[di] = q[i, j]
        cov[i, j] = True
    return SimpleNamespace(exp=pack(oc, tc), rn=rn, sc=sc, t_pre=t_pre, t=t, q=q, cov=cov,
                           shares=Shares(t, U, q, tc, cov))


def assert_finite(exp, code, what):
    """no NaN and no inf expected, so a NaN-tolerant comparison hides nothing"""
    assert np.isfinite(widen(exp, code)).all(), f"{what}: the expected buffer holds a NaN or an inf"
