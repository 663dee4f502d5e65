"""MXFP6 without a GPU, part 1: the numpy model's own arithmetic (fp6_common.py restates costa_hip.h,
"MXFP6") and the ABI: the header compiles as C and C++ with COSTA_FP6_E2M3 / COSTA_FP6_E3M2, the
library names the types and Python passes the codes through."""
import os
import subprocess

import numpy as np
import pytest

import fp6_common as f6
import mx_common as mc
from fp6_common import CEIL, COLS, E2M3, E3M2, FLOOR, FP6, ROWS, cvt6, pack, unpack, w6

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = pytest.mark.parametrize("p", FP6, ids=[f6.NAMES[p] for p in FP6])


# ------------------------------------------------------------------ the model
def test_pack_and_unpack_are_inverse():
    codes = np.random.default_rng(1).integers(0, 64, 4096).astype(np.uint8)
    b = pack(codes)
    assert b.size == 3072 and (unpack(b) == codes).all()
    # the first element in the lowest bits: w = c0 | c1 << 6 | c2 << 12 | c3 << 18, bytes low to high
    w = 0x01 | 0x22 << 6 | 0x13 << 12 | 0x3F << 18
    assert list(pack(np.array([0x01, 0x22, 0x13, 0x3F], np.uint8))) == [w & 0xFF, (w >> 8) & 0xFF, w >> 16]
    assert list(pack(np.array([0x3F, 0, 0, 0], np.uint8))) == [0x3F, 0, 0]
    assert list(pack(np.array([0, 0, 0, 0x3F], np.uint8))) == [0, 0, 0xFC]
    every = np.random.default_rng(2).integers(0, 256, 3 * 1000).astype(np.uint8)
    assert (pack(unpack(every)) == every).all()


@TYPES
def test_every_code_round_trips(p):
    codes = np.arange(64, dtype=np.uint8)
    v = w6(codes, p)
    if p == E2M3:
        assert list(v[:9]) == [0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0]
        assert list(v[24:32]) == [4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5]
    else:
        assert list(v[:8]) == [0, 0.0625, 0.125, 0.1875, 0.25, 0.3125, 0.375, 0.4375]
        assert list(v[24:32]) == [8, 10, 12, 14, 16, 20, 24, 28]
    assert (v[32:] == -v[:32]).all()
    assert np.signbit(v[32]) and v.view(np.uint32)[32] == 0x80000000
    assert v.view(np.uint32)[31] == f6.FMAX_BITS[p]
    assert v[1] == f6.MIN_SUBNORMAL[p] and f6.MIN_NORMAL[p] in v[:32]
    assert (cvt6(v, p) == codes).all()


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["pos", "neg"])
@TYPES
def test_the_thirty_one_ties_go_to_the_even_mantissa(p, sign):
    mags = f6.MAGS[p]
    ties = ((mags[:-1].astype(np.float64) + mags[1:]) / 2).astype(np.float32)
    assert ties.size == 31 and ((ties.astype(np.float64) * 2) == mags[:-1].astype(np.float64) + mags[1:]).all()
    k = np.arange(31, dtype=np.uint8)
    want = np.where(k % 2 == 0, k, k + 1).astype(np.uint8)             # the even code of k, k + 1
    assert (want % 2 == 0).all()
    s = 32 if sign < 0 else 0
    assert (cvt6(ties * np.float32(sign), p) == (want | s)).all()
    # one ulp to either side of a tie rounds to the nearer neighbour
    below = np.nextafter(ties, np.float32(0)) * np.float32(sign)
    above = np.nextafter(ties, np.float32(64)) * np.float32(sign)
    assert (cvt6(below, p) == (k | s)).all()
    assert (cvt6(above, p) == ((k + 1) | s)).all()


@TYPES
def test_zeros_and_values_rounding_to_zero_keep_their_sign(p):
    fm = f6.FMAX[p]
    t = np.array([-0.0, -0.01, -1e-30, 0.0, 0.01, np.nan, -fm, fm], np.float32)
    assert list(cvt6(t, p)) == [0x20, 0x20, 0x20, 0x00, 0x00, 0x00, 0x3F, 0x1F]
    assert cvt6(np.array([-np.nan], np.float32), p)[0] == 0x00
    half_step = f6.MIN_SUBNORMAL[p] / 2                                # the tie below the smallest subnormal: to 0
    assert list(cvt6(np.array([half_step, -half_step], np.float32), p)) == [0x00, 0x20]


@pytest.mark.parametrize("k", [-3, 0, 5])
@TYPES
def test_blocks_at_fmax_times_a_power_of_two(p, k):
    """a maximum of exactly fmax * 2^k scales onto fmax under both rules; one ulp above saturates under
    FLOOR and raises E under CEIL"""
    fm, emax = f6.FMAX[p], f6.EMAX[p]
    top = fm * np.float32(2.0) ** k
    above = np.nextafter(top, np.float32(np.inf))
    V = np.zeros((32, 2), np.float32)
    V[:, 0] = np.linspace(-1, 1, 32, dtype=np.float32) * top / 8
    V[:, 1] = V[:, 0]
    V[4, 0], V[4, 1] = top, above
    E_floor = 127 + k                                                  # e of fmax * 2^k is 127 + k + emax
    q, E, t = f6.quantise_dense6(V, ROWS, p, FLOOR)
    assert list(E[0]) == [E_floor, E_floor] and emax == int(np.floor(np.log2(fm)))
    assert t[4, 0] == fm and t[4, 1] > fm and q[4, 0] == 0x1F and q[4, 1] == 0x1F     # the clamp
    q2, E2, t2 = f6.quantise_dense6(V, ROWS, p, CEIL)
    assert list(E2[0]) == [E_floor, E_floor + 1]
    assert (np.abs(t2) <= fm).all() and q2[4, 0] == 0x1F and t2[4, 1] > fm / 2
    assert q2[4, 1] == cvt6(np.array([fm / 2], np.float32), p)[0]      # half of fmax, rounded by the type
    # the same blocks along columns
    q3, E3, _ = f6.quantise_dense6(V.T.copy(), COLS, p, FLOOR)
    assert (q3 == q.T).all() and (E3 == E).all()


@TYPES
def test_special_blocks_in_the_model(p):
    emax = f6.EMAX[p]
    V = np.zeros((32, 6), np.float32)
    V[2, 0] = -0.0
    V[9, 1] = np.nan
    V[9, 2] = -np.inf
    V[:, 3] = np.float32(1e-42)                                        # below 2^-125: E clamps to 0
    V[:, 4] = np.float32(2.5e38)
    V[7, 5] = 1.0                                                      # amax 2^0: E = 127 - emax, q = 2^emax
    q, E, t = f6.quantise_dense6(V, ROWS, p, FLOOR)
    assert list(E[0]) == [0, 255, 255, 0, 254 - emax, 127 - emax]
    assert q[2, 0] == 0x20 and (np.delete(q[:, 0], 2) == 0).all()
    assert (q[:, 1] == 0).all() and (q[:, 2] == 0).all()               # E = 255: code 0x00 everywhere
    assert w6(q[7, 5], p) == 2.0 ** emax and (q[:, 4] == q[0, 4]).all()


@TYPES
def test_the_oracle_moves_all_sixty_four_values_bit_for_bit(p):
    """gather / place of mx_common keep -0.0, so pack(cvt6(place(w6(..)))) is exact for old contents"""
    a_case, _ = f6.geometry("custom32q", "N")
    n = a_case.buf_elems(0, 1)
    assert n % 4 == 0
    codes = np.resize(np.arange(64, dtype=np.uint8), n)
    dense = mc.gather(a_case, 1, [w6(codes, p)])
    back = mc.place(a_case, 1, dense, [np.zeros(n, np.float32)])[0]
    m, k = a_case.shape()
    assert np.signbit(dense).sum() > 0
    own = mc.place(a_case, 1, np.ones((m, k), np.float32), [np.zeros(n, np.float32)])[0] == 1.0
    assert (cvt6(back, p)[own] == codes[own]).all()


def test_the_issue_saturation_counts():
    """quant_data at 204 x 156, seed 0x31: the counts of elements above fmax before the clamp"""
    V = mc.quant_data(0x31, 204 * 156).reshape(156, 204).T.copy()
    want = {(E2M3, ROWS): 1208, (E2M3, COLS): 227, (E3M2, ROWS): 2446, (E3M2, COLS): 472}
    for (p, axis), n in want.items():
        _, _, t = f6.quantise_dense6(V, axis, p, FLOOR)
        assert int((np.abs(t) > f6.FMAX[p]).sum()) == n, (p, axis)
        _, _, t = f6.quantise_dense6(V, axis, p, CEIL)
        assert int((np.abs(t) > f6.FMAX[p]).sum()) == 0


# ------------------------------------------------------------------ the ABI
PROG = r'''
#include "costa_hip.h"
int main(void) {
    costa_dtype_t a = COSTA_FP6_E2M3, b = COSTA_FP6_E3M2;
    return (int)a == 10 && (int)b == 11 && (int)COSTA_FP4_E2M1 == 9 && sizeof(costa_mx_scales_t) == 32 ? 0 : 1;
}
'''


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_with_the_new_constants(tmp_path, lang):
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text(PROG)
    exe = tmp_path / "t"
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


@TYPES
def test_dtype_name_and_element_code(costa, p):
    assert (costa.FP6_E2M3, costa.FP6_E3M2) == (E2M3, E3M2) == (10, 11)
    assert "FP6_E2M3" in costa.__all__ and "FP6_E3M2" in costa.__all__ and costa.FP4_E2M1 == 9
    assert costa.element_code(p) == p and costa.np_dtype(p) == np.uint8
    with pytest.raises(ValueError):
        costa.dtype_code(np.uint8)                                     # a plain byte array is not an FP6 matrix
    # the library's name of the type, through a refusal that prints it
    a_case, c_case = f6.geometry("g204", "N")
    A = f6.make_layout(costa, a_case, 0, 1 << 40, 1, p)
    C = f6.make_layout(costa, c_case, 0, 1 << 41, 1, p)
    with pytest.raises(costa.CostaError, match=f6.TYPE_NAMES[p]) as ei:
        costa.plan_export([A], [C], 0, 1)
    assert ei.value.code == 1
