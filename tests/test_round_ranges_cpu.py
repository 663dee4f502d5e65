"""The exchange rounds of a peer's package, through the host-only exports costa_hip_exchange_rounds and
costa_hip_round_range (no GPU): the ranges issue_exchange moves per round and the driver of
tests/emulated_ranks.py copies.

A package of n elements of E bytes moves in one part below the threshold (16 MiB) and in R equal
parts at or above it; round r of R moves [n*r/parts, n*(r+1)/parts), and rounds past the parts are
empty at n.  Both sides of a pair derive this from the pair's count alone."""
import os
import subprocess
import sys

import pytest

THRESHOLD = 16 << 20  # kRoundMinBytes (engine.cpp); COSTA_ROUND_MIN_BYTES is a tuning override
ELEM = (1, 2, 4, 8, 16)
ROUNDS = tuple(range(1, 17))


def counts(E):
    at = THRESHOLD // E
    return [0, 1, 3, 12345, at - 1, at, at + 1, 2 * at + 7, 1048577 * 3, (1 << 31) + 7]


@pytest.fixture(scope="module")
def lib(costa):
    return costa


def test_exchange_rounds_default(lib):
    R = lib.exchange_rounds()
    assert 1 <= R <= 16
    if "COSTA_EXCHANGE_ROUNDS" not in os.environ:
        assert R == 4


@pytest.mark.parametrize("E", ELEM)
def test_ranges_tile_the_package(lib, E):
    """the R ranges tile [0, n) in order, in 1 part below the threshold and R parts at or above it,
    and every round past the parts is empty at n"""
    for n in counts(E):
        for R in ROUNDS:
            parts = R if n * E >= THRESHOLD else 1
            at = 0
            for r in range(parts):
                lo, hi = lib.round_range(n, E, R, r)
                assert lo == at and lo <= hi <= n, (n, E, R, r, lo, hi)
                # equal parts: sizes differ by at most one element
                assert n // parts <= hi - lo <= -(-n // parts), (n, E, R, r, lo, hi)
                at = hi
            assert at == n, (n, E, R)
            for r in list(range(parts, R)) + [R, R + 3]:
                assert lib.round_range(n, E, R, r) == (n, n), (n, E, R, r)


@pytest.mark.parametrize("E", ELEM)
def test_threshold_is_in_bytes(lib, E):
    at = THRESHOLD // E
    assert lib.round_range(at - 1, E, 4, 0) == (0, at - 1)
    assert lib.round_range(at, E, 4, 0) == (0, at // 4)
    assert lib.round_range(at, E, 4, 3) == (3 * at // 4, at)


def test_bad_arguments(lib):
    for args in ((-1, 4, 4, 0), (10, 0, 4, 0), (10, 4, 0, 0), (10, 4, 4, -1)):
        with pytest.raises(lib.CostaError) as e:
            lib.round_range(*args)
        assert e.value.code == 1


def test_family_geometries_cover_every_part():
    """the FP8 family of tests/emulated_family_child.py (1-byte packages: the smallest) on the host
    only: on every rank of every case the plan sends, receives and has a LOCAL list, and some
    off-rank package of at least 2048 bytes moves in 4 parts"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, COSTA_TUNING="1", COSTA_ROUND_MIN_BYTES="2048")
    r = subprocess.run([sys.executable, os.path.join(here, "emulated_family_child.py"), "fp8", "--dry"],
                       env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, multi = out[-1].split()
    assert int(n) == 12 and int(multi) >= 12, out[-1]


@pytest.mark.parametrize("tuning,parts", [("1", 4), ("0", 1), (None, 1)])
def test_threshold_override_needs_tuning(tuning, parts):
    """COSTA_ROUND_MIN_BYTES is read through the tuning switch, once per process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import costa_amd as c; "
            "print(sum(1 for r in range(4) if (lambda a, b: b > a)(*c.round_range(2048, 1, 4, r))), "
            "c.round_range(2047, 1, 4, 0))" % root)
    env = {k: v for k, v in os.environ.items() if k not in ("COSTA_TUNING", "COSTA_ROUND_MIN_BYTES")}
    env.update(COSTA_ROUND_MIN_BYTES="2048", COSTA_NO_TORCH="1")
    if tuning is not None:
        env["COSTA_TUNING"] = tuning
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"{parts} (0, 2047)", r.stdout + r.stderr
