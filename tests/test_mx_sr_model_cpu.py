"""The model of stochastic rounding in the MX transforms (mx_sr_common.py; costa_hip.h, "Stochastic
rounding in the MX transforms") and the host function costa_hip_sr_bits, without a GPU: known answers
of the hash, the conversion on representable values and hand cases, its bias over fixed seeds, and
the hash as a field of random bits over the positions of a matrix."""
import numpy as np
import pytest

import fp4_common as f4
import mx_sr_common as sr
from mx_sr_common import E2M3, E3M2, E4M3, E5M2, FP4, M24, NAMES, QTYPES

TYPES = pytest.mark.parametrize("tq", QTYPES, ids=[NAMES[t] for t in QTYPES])
SEED = 0x0123456789ABCDEF
POS = [(0, 0), (1, 2), (202, 157), (70000, 3)]
U_SEED = [0x40042D, 0x0C4B6B, 0x09E145, 0x0982E5]
U_ZERO = [0x2D3D8A, 0xECE447, 0x5F71F2, 0x40208F]


# ------------------------------------------------------------------ known answers
def test_known_answers_of_the_model():
    assert int(sr.fmix32(1)) == 0x514E28B7
    assert sr.keys(0) == (0x92CA2F0E, 0xCB72770F)
    assert sr.keys(SEED) == (0x089887A8, 0x66EA390A)
    assert [int(sr.rand24(SEED, i, j)) for i, j in POS] == U_SEED
    assert [int(sr.rand24(0, i, j)) for i, j in POS] == U_ZERO


def test_known_answers_of_sr_bits(costa):
    assert [costa.sr_bits(SEED, i, j) for i, j in POS] == U_SEED
    assert [costa.sr_bits(0, i, j) for i, j in POS] == U_ZERO


def test_sr_bits_equals_the_model(costa):
    rng = np.random.default_rng(0x5B)
    n = 10000
    seeds = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    i = rng.integers(0, 1 << 31, n, dtype=np.int64)
    j = rng.integers(0, 1 << 31, n, dtype=np.int64)
    i[:4], j[:4] = (0, (1 << 31) - 1, 0, (1 << 31) - 1), (0, 0, (1 << 31) - 1, (1 << 31) - 1)
    assert (seeds > np.uint64(1 << 32)).sum() > n // 2
    for s, a, b in zip(seeds.tolist(), i.tolist(), j.tolist()):
        u = costa.sr_bits(s, a, b)
        assert u == int(sr.rand24(s, a, b)) and 0 <= u < M24, (s, a, b)


def test_python_seed_check(costa):
    for bad in (-1, 1 << 64, 1.5, "7", None):
        with pytest.raises(ValueError):
            costa.sr_bits(bad, 0, 0)
    assert costa.sr_bits((1 << 64) - 1, 0, 0) == int(sr.rand24((1 << 64) - 1, 0, 0))


# ------------------------------------------------------------------ the conversion
@TYPES
def test_representable_values_convert_to_themselves(tq):
    n = sr.mags(tq).size
    codes = np.concatenate([np.arange(n, dtype=np.uint8), np.arange(n, dtype=np.uint8) | np.uint8(sr.SIGN[tq])])
    t = sr.widen_codes(codes, tq)
    for U in (0, M24 - 1):
        assert (sr.sr_codes(t, U, tq) == codes).all()
    assert (sr.rn_codes(t, tq) == codes).all()


def _one(t, U, tq):
    return int(sr.sr_codes(np.array([t], np.float32), U, tq)[0])


def test_hand_cases():
    # e2m1: 1.25 lies half way between 1.0 (code 2) and 1.5 (code 3)
    assert _one(1.25, 0x7FFFFF, FP4) == 2 and _one(1.25, 0x800000, FP4) == 3
    assert float(f4.w4(2)) == 1.0 and float(f4.w4(3)) == 1.5
    # e4m3: 2^-10 is half a subnormal step (2^-9): the same two U split it
    assert _one(2.0 ** -10, 0x7FFFFF, E4M3) == 0 and _one(2.0 ** -10, 0x800000, E4M3) == 1
    for tq in QTYPES:
        s = sr.SIGN[tq]
        for U in (0, 1, 0x800000, M24 - 1):
            # 2^-40: T = 0, never up -- except e5m2, whose subnormal step is 2^-16: T = 2^(-40 + 16 + 24) = 1,
            # up for the one U = 2^24 - 1
            up = int(tq == E5M2 and U == M24 - 1)
            assert _one(2.0 ** -40, U, tq) == up
            assert _one(2.0 ** -41, U, tq) == 0
            assert _one(-0.0, U, tq) == s                   # the sign bit is kept
            assert _one(-2.0 ** -40, U, tq) == s | up
    for U in (0, 1, 0x7FFFFF, 0x800000, M24 - 1):
        assert _one(448.0, U, E4M3) == 0x7E and _one(-448.0, U, E4M3) == 0xFE
        assert _one(6.0, U, FP4) == 7 and _one(-6.0, U, FP4) == 15
    # the probability is T / 2^24 exactly: 1.0 + 2^-23 in e2m1 has T = 2^-22 * 2^24 = 4 of 2^24
    x = np.float32(1.0) + np.float32(2.0 ** -23)
    assert _one(x, M24 - 5, FP4) == 2 and _one(x, M24 - 4, FP4) == 3
    # a NaN (a block with E = 255): the NaN code of FP8, code 0 of FP4 / FP6
    assert [_one(np.nan, 5, tq) for tq in QTYPES] == [0x7F, 0x7F, 0, 0, 0]


@TYPES
@pytest.mark.parametrize("seed", [0, 1, 99])
def test_bias_is_within_four_sigma(tq, seed):
    """|sum(w(q) - t)| <= 4 sqrt(sum f (1 - f) step^2), f = T / 2^24: SR is unbiased; on the same data
    round-to-nearest is not asked anything (its error is deterministic)"""
    fm = float(sr.FMAX[tq])
    rng = np.random.default_rng(1000 + seed)
    t = sr.clamp(rng.uniform(-1.1 * fm, 1.1 * fm, (256, 256)).astype(np.float32), tq)
    q = sr.sr_codes(t, sr.rand24_grid(seed, 256, 256), tq)
    _, T, step = sr.sr_parts(t, tq)
    f = T / float(M24)
    err = (sr.widen_codes(q, tq).astype(np.float64) - t.astype(np.float64)).sum()
    sigma = np.sqrt((f * (1 - f) * step ** 2).sum())
    print(f"{NAMES[tq]} seed {seed}: z = {err / sigma:+.3f}")
    assert abs(err) <= 4 * sigma


def test_constant_between_two_codes():
    """256 x 256 of 1.25 in e2m1, seed 7: half goes to 1.5 (4 sigma = 4 * 0.5 / 256 = 0.0078); the
    round-to-nearest model sends none there"""
    t = np.full((256, 256), 1.25, np.float32)
    q = sr.sr_codes(t, sr.rand24_grid(7, 256, 256), FP4)
    assert set(np.unique(q)) == {2, 3}
    share = float((q == 3).mean())
    print(f"share rounded to 1.5: {share:.4f}")
    assert abs(share - 0.5) <= 4 * 0.5 / 256
    assert (sr.rn_codes(t, FP4) == 2).all()
    # the sum: SR keeps it within 4 sigma of 1.25 * 65536, round-to-nearest loses 0.25 per element
    assert abs(float(f4.w4(q).astype(np.float64).sum()) - 1.25 * 65536) <= 4 * 0.25 * 256
    assert float(f4.w4(sr.rn_codes(t, FP4)).sum()) == 65536.0


# ------------------------------------------------------------------ the hash as a field
FIELD_SEEDS = [0, 1, 2, 12345, 1 << 32, (1 << 63) + 5, (1 << 64) - 1]
GRIDS = [(256, 256, 0, 0), (64, 1024, 1000, 5), (1024, 64, 7, 100000)]
PROBS = [1 / 16, 1 / 4, 3 / 8, 1 / 2, 5 / 8, 15 / 16]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}at{g[2]},{g[3]}")
@pytest.mark.parametrize("seed", FIELD_SEEDS, ids=lambda s: f"{s:#x}")
def test_hash_field(seed, grid):
    """for T / 2^24 = p the up decisions T + U >= 2^24 are a Bernoulli(p) field: the share of ups and the
    lag-1 correlations along rows, columns and the diagonal stay within 4 sigma (sigma of a share of n
    trials: sqrt(p (1 - p) / n); of a lag-1 correlation of n pairs: 1 / sqrt(n))"""
    m, n, i0, j0 = grid
    U = sr.rand24_grid(seed, m, n, i0, j0).astype(np.int64)
    worst = 0.0
    for p in PROBS:
        T = int(p * M24)
        up = (T + U >= M24).astype(np.float64)
        z = [(up.mean() - p) / np.sqrt(p * (1 - p) / up.size)]
        d = (up - p) / np.sqrt(p * (1 - p))
        for a, b in ((d[:, :-1], d[:, 1:]), (d[:-1, :], d[1:, :]), (d[:-1, :-1], d[1:, 1:])):
            z.append((a * b).mean() * np.sqrt(a.size))
        worst = max(worst, max(abs(x) for x in z))
        assert max(abs(x) for x in z) <= 4, (p, z)
    print(f"seed {seed:#x} grid {grid}: worst |z| = {worst:.2f}")
