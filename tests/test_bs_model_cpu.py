"""The model of the block-scaled FP8 transforms (bs_common.py) checked against the statements of
costa_hip.h, "Block-scaled FP8 transforms (fp32 scales)", without a GPU."""
import numpy as np
import pytest

import bs_common as bc
from bs_common import E4M3, E5M2, EXACT, POW2, SHAPES, SHAPE_IDS

QS = [E4M3, E5M2]


def _codes_at_top(tq):
    """the bit patterns of +fmax and of the code just below"""
    top = int(bc.cvt(np.array([bc.FMAX[tq]], np.float32), tq)[0])
    return top, top - 1


@pytest.mark.parametrize("block", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("tq", QS, ids=lambda c: bc.NAMES[c])
def test_exact_amax_element_lands_on_fmax_or_just_below(tq, block):
    V = bc.quant_data(0x11, bc.M * bc.N).reshape(bc.M, bc.N)
    q, S, t = bc.quantise_dense(V, block, tq, EXACT)
    assert S.shape == bc.n_blocks(V.shape, block) and np.isfinite(S).all() and (S > 0).all()
    top, below = _codes_at_top(tq)
    amax = bc.block_amax_bits(V, block)
    at_max = (np.ascontiguousarray(V).view(np.uint32) & np.uint32(0x7FFFFFFF)) == bc.expand(
        amax.view(np.float32), block, *V.shape).view(np.uint32)
    assert at_max.sum() >= S.size
    mag = q[at_max] & 0x7F
    assert np.isin(mag, [top, below]).all()
    assert (np.abs(bc.widen(q.reshape(-1), tq)) <= float(bc.FMAX[tq])).all()
    # S is numpy's fp32 quotient, bit for bit
    assert (S.view(np.uint32) == (amax.view(np.float32) / bc.FMAX[tq]).view(np.uint32)).all()


@pytest.mark.parametrize("block", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("tq", QS, ids=lambda c: bc.NAMES[c])
def test_pow2_scales_are_powers_of_two_and_nothing_is_clamped(tq, block):
    V = bc.quant_data(0x12, bc.M * bc.N).reshape(bc.M, bc.N)
    q, S, t = bc.quantise_dense(V, block, tq, POW2)
    assert (S.view(np.uint32) & np.uint32(0x807FFFFF) == 0).all() and (S.view(np.uint32) != 0).all()
    fm = float(bc.FMAX[tq])
    assert (np.abs(t) <= fm).all()
    # ... and the scale is the smallest such power of two: half of it would overflow
    amax = bc.block_amax_bits(V, block).view(np.float32)
    assert (amax / (S * np.float32(0.5)) > fm).all()
    # dequantised, every element is within half a step of the block's grid
    back = bc.widen(q.reshape(-1), tq).reshape(V.shape) * bc.expand(S, block, *V.shape)
    step = bc.expand(S, block, *V.shape) * np.float32(2.0 ** (bc.EMAX[tq] - (3 if tq == E4M3 else 2)))
    assert (np.abs(back - V) <= step / 2).all()


@pytest.mark.parametrize("rounding", [EXACT, POW2], ids=["exact", "pow2"])
@pytest.mark.parametrize("tq", QS, ids=lambda c: bc.NAMES[c])
def test_special_blocks(tq, rounding):
    fm = bc.FMAX[tq]
    V = bc.special_matrix()
    q, S, t = bc.quantise_dense(V, (128, 1), tq, rounding)
    assert S.shape == (1, 8)
    eps = np.float32(2.0 ** -40)
    floor = (eps / fm) if rounding == EXACT else None
    w = bc.widen(q.reshape(-1), tq).reshape(V.shape)
    # all-zero, below 2^-40, subnormal: the eps clamp decides the scale
    for col in (0, 1, 2):
        if rounding == EXACT:
            assert S[0, col].view(np.uint32) == floor.view(np.uint32)
        else:  # 2^-40 * 2^emax <= fmax: the ceil rule adds nothing
            assert S[0, col] == np.float32(2.0 ** (-40 - bc.EMAX[tq]))
        assert np.isfinite(w[:, col]).all()
    assert (q[:, 0] == 0).all()
    assert q[2, 5] == 0x80 and (np.delete(q[:, 5], 2) == 0).all()          # -0 keeps its sign
    # an inf or a NaN in the block: S = NaN (0x7FC00000), every q a NaN
    for col in (3, 4):
        assert S[0, col].view(np.uint32) == 0x7FC00000 and np.isnan(w[:, col]).all()
    # the largest and the smallest normal amax stay finite and normal in S
    for col in (6, 7):
        assert np.isfinite(S[0, col]) and S[0, col] >= np.float32(2.0 ** -126) and np.isfinite(w[:, col]).all()


def test_exact_clamp_is_load_bearing():
    """some amax * R rounds above fmax under EXACT: without the clamp e4m3 would give a NaN"""
    rng = np.random.default_rng(3)
    a = rng.uniform(1.0, 2.0, 20000).astype(np.float32)
    over = a * (bc.FMAX[E4M3] / a) > bc.FMAX[E4M3]
    assert over.any()
    V = np.zeros((128, 1), np.float32)
    V[5, 0] = a[np.flatnonzero(over)[0]]
    q, S, t = bc.quantise_dense(V, (128, 1), E4M3, EXACT)
    assert t[5, 0] > 448.0 and q[5, 0] == 0x7E


def test_partial_blocks_reduce_over_existing_elements():
    V = bc.quant_data(0x13, 130 * 129).reshape(130, 129)
    for block in SHAPES:
        S = bc.quantise_dense(V, block, E4M3, EXACT)[1]
        nbr, nbc = bc.n_blocks(V.shape, block)
        last = np.abs(V[(nbr - 1) * block[0]:, (nbc - 1) * block[1]:]).max()
        assert S[-1, -1] == np.float32(last) / np.float32(448.0)
