"""MXFP4 without a GPU, part 1: the numpy model's own arithmetic (fp4_common.py restates costa_hip.h,
"MXFP4") and the ABI: the header compiles as C and C++ with COSTA_FP4_E2M1, the library names the type
and Python maps torch.float4_e2m1fn_x2 to it."""
import os
import subprocess

import numpy as np
import pytest

import fp4_common as f4
import mx_common as mc
from fp4_common import CEIL, COLS, FLOOR, FP4, ROWS, cvt4, pack, unpack, w4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the model
def test_pack_and_unpack_are_inverse():
    codes = np.random.default_rng(1).integers(0, 16, 4096).astype(np.uint8)
    b = pack(codes)
    assert b.size == 2048 and (unpack(b) == codes).all()
    assert pack(np.array([0x3, 0xA], np.uint8))[0] == 0xA3      # even index in bits 3..0: hi << 4 | lo
    every = np.arange(256, dtype=np.uint8)
    assert (pack(unpack(every)) == every).all()


def test_every_code_round_trips():
    codes = np.arange(16, dtype=np.uint8)
    v = w4(codes)
    assert list(v[:8]) == [0, 0.5, 1, 1.5, 2, 3, 4, 6] and list(v[8:]) == [-0.0, -0.5, -1, -1.5, -2, -3, -4, -6]
    assert np.signbit(v[8]) and v.view(np.uint32)[8] == 0x80000000
    assert (cvt4(v) == codes).all()


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["pos", "neg"])
def test_the_seven_ties_go_to_the_even_mantissa(sign):
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32) * np.float32(sign)
    want = np.array([0, 2, 2, 4, 4, 6, 6], np.uint8) | (8 if sign < 0 else 0)
    assert (cvt4(ties) == want).all()
    # one ulp to either side of a tie rounds to the nearer neighbour
    below = np.nextafter(np.abs(ties), np.float32(0)) * np.float32(sign)
    above = np.nextafter(np.abs(ties), np.float32(8)) * np.float32(sign)
    s = 8 if sign < 0 else 0
    assert (cvt4(below) == (np.arange(7, dtype=np.uint8) | s)).all()
    assert (cvt4(above) == (np.arange(1, 8, dtype=np.uint8) | s)).all()


def test_zeros_and_values_rounding_to_zero_keep_their_sign():
    t = np.array([-0.0, -0.2, -0.25, -1e-30, 0.0, 0.2, np.nan, -6.0, 6.0], np.float32)
    assert list(cvt4(t)) == [0x8, 0x8, 0x8, 0x8, 0x0, 0x0, 0x0, 0xF, 0x7]
    assert cvt4(np.array([-np.nan], np.float32))[0] == 0x0


@pytest.mark.parametrize("k", [-3, 0, 5])
def test_blocks_at_six_times_a_power_of_two(k):
    """a maximum of exactly 6 * 2^k scales onto 6.0 under both rules; one ulp above saturates under FLOOR
    and raises E under CEIL"""
    six = np.float32(6.0) * np.float32(2.0) ** k
    above = np.nextafter(six, np.float32(np.inf))
    V = np.zeros((32, 2), np.float32)
    V[:, 0] = np.linspace(-1, 1, 32, dtype=np.float32) * six / 8
    V[:, 1] = V[:, 0]
    V[4, 0], V[4, 1] = six, above
    E_floor = 127 + k + 2 - f4.EMAX4                                   # e of 6 * 2^k is 127 + k + 2
    q, E, t = f4.quantise_dense4(V, ROWS, FLOOR)
    assert list(E[0]) == [E_floor, E_floor]
    assert t[4, 0] == 6.0 and t[4, 1] > 6.0 and q[4, 0] == 0x7 and q[4, 1] == 0x7   # the clamp
    q2, E2, t2 = f4.quantise_dense4(V, ROWS, CEIL)
    assert list(E2[0]) == [E_floor, E_floor + 1]
    assert (np.abs(t2) <= 6.0).all() and q2[4, 0] == 0x7 and q2[4, 1] == 0x5 and t2[4, 1] > 3.0
    # the same blocks along columns
    q3, E3, _ = f4.quantise_dense4(V.T.copy(), COLS, FLOOR)
    assert (q3 == q.T).all() and (E3 == E).all()


def test_special_blocks_in_the_model():
    V = np.zeros((32, 6), np.float32)
    V[2, 0] = -0.0
    V[9, 1] = np.nan
    V[9, 2] = -np.inf
    V[:, 3] = np.float32(1e-42)                                        # below 2^-125: E clamps to 0
    V[:, 4] = np.float32(2.5e38)
    V[7, 5] = 1.0                                                      # amax 2^0: E = 125, q = 4.0
    q, E, t = f4.quantise_dense4(V, ROWS, FLOOR)
    assert list(E[0]) == [0, 255, 255, 0, 254 - f4.EMAX4, 127 - f4.EMAX4]
    assert q[2, 0] == 0x8 and (np.delete(q[:, 0], 2) == 0).all()
    assert (q[:, 1] == 0).all() and (q[:, 2] == 0).all()               # E = 255: code 0x0 everywhere
    assert q[7, 5] == 0x6 and (q[:, 4] == q[0, 4]).all()


def test_the_oracle_moves_all_sixteen_values_bit_for_bit():
    """gather / place of mx_common keep -0.0, so pack(cvt4(place(w4(..)))) is exact for old contents"""
    a_case, _ = f4.geometry("custom32", "N")
    n = a_case.buf_elems(0, 1)
    codes = np.resize(np.arange(16, dtype=np.uint8), n)
    dense = mc.gather(a_case, 1, [w4(codes)])
    back = mc.place(a_case, 1, dense, [np.zeros(n, np.float32)])[0]
    m, k = a_case.shape()
    assert (cvt4(dense) < 16).all() and np.signbit(dense).sum() > 0
    own = mc.place(a_case, 1, np.ones((m, k), np.float32), [np.zeros(n, np.float32)])[0] == 1.0
    assert (cvt4(back)[own] == codes[own]).all()


# ------------------------------------------------------------------ the ABI
PROG = r'''
#include "costa_hip.h"
int main(void) {
    costa_dtype_t t = COSTA_FP4_E2M1;
    return (int)t == 9 && (int)COSTA_FP8_E5M2 == 8 && sizeof(costa_mx_scales_t) == 32 ? 0 : 1;
}
'''


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_with_the_new_constant(tmp_path, lang):
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text(PROG)
    exe = tmp_path / "t"
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_dtype_name_and_element_code(costa):
    assert costa.FP4_E2M1 == FP4 == 9 and "FP4_E2M1" in costa.__all__
    assert costa.element_code(FP4) == FP4 and costa.np_dtype(FP4) == np.uint8
    # torch's dtype object is recognised by module and name (no torch import, any torch version)
    fake = type("dtype", (), {"__module__": "torch", "__str__": lambda self: "torch.float4_e2m1fn_x2"})()
    assert costa.element_code(fake) == FP4
    with pytest.raises(ValueError):
        costa.dtype_code(np.uint8)                                     # a plain byte array is not an FP4 matrix
    # the library's name of the type, through a refusal that prints it
    a_case, c_case = f4.geometry("g202", "N")
    A = f4.make_layout(costa, a_case, 0, 1 << 40, 1, FP4)
    C = f4.make_layout(costa, c_case, 0, 1 << 41, 1, FP4)
    with pytest.raises(costa.CostaError, match="FP4_E2M1") as ei:
        costa.plan_export([A], [C], 0, 1)
    assert ei.value.code == 1
