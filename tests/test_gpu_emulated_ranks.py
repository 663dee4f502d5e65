"""Multi-rank transforms on ONE GPU through the code a real N > 1 transform() runs: the per-round
pack / unpack lists (list_pack / list_unpack, exchange_round_of_ops / _tri / _scaled, the cv_pack /
cv_unpack choice) launched against package buffers, with tests/emulated_ranks.py as the exchange.
test_gpu_parity.py, test_gpu_multiproc.py and test_gpu_tri.py run the same plans through
costa_hip_execute_tiles*, whose lists are all of the default kind and never split into rounds.

Packages start as 0xFF bytes (NaN in every floating type) and arrive round by round, so an op in
the wrong round, a lost op or a wrong piece cut shows in the destination; expected values are
therefore checked to be finite, except in the specials cases.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from cases import all_cases, special_cases
from casegen import Custom
from emulated_ranks import alg_bytes, dev, drive, pair_parts, poisoned
from golden_io import first_mismatch, load, matches
from test_gpu_parity import assert_bits_equal_or_both_nan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
# golden cases on several ranks whose plans move nothing between ranks (identical source and target
# distributions, or a matrix of a single block): no pack or unpack list exists, only LOCAL runs
NO_EXCHANGE = {"cfg1", "sweep_23", "sweep_28", "specials_z_2r"}
FAMILY_CASES = {"plain": 16, "half": 12, "fp8": 12, "tri": 8, "scaled": 21, "amax": 8}


@pytest.fixture(scope="module")
def gpu(costa):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return costa


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


# ------------------------------------------------------------------ a. golden cases, b. statistics
MULTI = [c for c in all_cases() + special_cases() if c.P > 1]


def run_case(costa, case, local_first):
    """every rank's transform_batch of a golden case through the driver; ([rank][pair] -> C, plans,
    outcome)"""
    P, dt, K = case.P, oracle.NP[case.dtype], len(case.pairs)
    bufs = [[tuple(dev(x) for x in case.inputs(k, r)) for k in range(K)] for r in range(P)]
    eff = [case.effective(k) for k in range(K)]
    tr, al, be = ([e[i] for e in eff] for i in range(3))
    lay, plans = [], []
    for r in range(P):
        As = [case.layout_A(k, r, bufs[r][k][0].data_ptr()) for k in range(K)]
        Cs = [case.layout_C(k, r, bufs[r][k][1].data_ptr()) for k in range(K)]
        lay.append((As, Cs))
        plans.append(costa.plan_export(As, Cs, r, P, tr, al, be))

    def call(r, comm):
        costa.transform_batch(lay[r][0], lay[r][1], comm, tr, al, be)

    out = drive(costa, plans, np.dtype(dt).itemsize, call, local_first=local_first)
    return [[host(bufs[r][k][1], dt) for k in range(K)] for r in range(P)], plans, out


@pytest.mark.parametrize("case", MULTI, ids=lambda c: c.name)
def test_golden_through_pack_unpack(gpu, case):
    """bit for bit against the reference's fixtures, the relabelled and batch cases included; and the
    statistics show that the product's pack / unpack lists ran, with the plan's byte counts"""
    fx = load(case.name)
    special = any(p.specials for p in case.pairs)
    E = np.dtype(oracle.NP[case.dtype]).itemsize
    got, plans, out = run_case(gpu, case, local_first=MULTI.index(case) % 2 == 1)
    for r in range(case.P):
        for k in range(len(case.pairs)):
            key = f"C{k}_r{r}"
            if special:
                assert_bits_equal_or_both_nan(got[r][k], fx[key])
                continue
            if key in fx:
                assert np.isfinite(fx[key]).all()
            assert matches(fx, key, got[r][k]), f"{case.name} {key}: " + first_mismatch(fx, key, got[r][k])
    st = out.stats
    moves = sum(p.send_elems for p in plans) > 0
    assert moves == (case.name not in NO_EXCHANGE)
    if moves:
        assert st["pack_launches"] > 0 and st["unpack_launches"] > 0, st
    else:
        assert st["pack_launches"] == 0 and st["unpack_launches"] == 0, st
    assert st["pack_bytes"] == sum(alg_bytes(p.pack_ops, E, E) for p in plans), st
    assert st["unpack_bytes"] == sum(alg_bytes(p.unpack_ops, E, E) for p in plans), st
    assert st["local_launches"] == sum(1 for p in plans if p.local_ops.size), st
    if case.name in ("cfg5_N", "cfg5_T"):  # unpack lists group by destination block, pack lists never do
        assert st["cblock_items"] > 0, st


# ------------------------------------------------------------------ c. the default threshold
def _straddled(costa, ops, key, displs, counts, me, E, R):
    """how many round cuts of the off-rank pairs fall strictly inside an op's package extent"""
    first = ops[key].astype(np.int64) // E
    last = first + ops["nf"].astype(np.int64) * ops["ns"].astype(np.int64)
    n = 0
    for q in range(len(counts)):
        if q == me:
            continue
        for r in range(1, R):
            cut = int(displs[q]) + costa.round_range(int(counts[q]), E, R, r)[0]
            n += bool(((first < cut) & (cut < last)).any())
    return n


def test_default_threshold_c128(gpu):
    """complex<double> 2048 x 2048 'C' on 2 ranks with alpha, beta, at the default 16 MiB threshold.
    A on a 1 x 2 grid (panels of 512 columns, dealt out in turn), C on a 2 x 1 grid (1024 rows each),
    both cut into blocks of 96 x 80 (a shorter first block, and a boundary where the owner changes):
    C's rows of one rank are two panels of A's columns, one of either rank, so each off-rank package
    is 2048 x 512 elements = exactly 16 MiB and moves in 4 parts.  The cuts (multiples of 262144
    elements) fall strictly inside ops, whose package extents are the ragged intersections of A's and
    C's blocks, at most 80 x 80 elements.  Expected: oracle.transform over both ranks' buffers."""
    assert gpu.exchange_rounds() == 4  # (the default; COSTA_EXCHANGE_ROUNDS unset)
    n, P, dt = 2048, 2, oracle.CDOUBLE
    alpha, beta = 0.75 - 0.5j, 1.25 + 0.25j

    def split(b, extra):  # (a shorter first block: with boundaries at 0 mod 16 on both sides the
        first = {96: 40, 80: 24}[b]  # package's first two cuts coincide with op boundaries)
        return sorted({0} | set(range(first, n, b)) | set(extra) | {n})
    ars, acs = split(96, ()), split(80, (512, 1024, 1536))
    crs, ccs = split(96, (1024,)), split(80, ())
    a_own = np.repeat(((np.array(acs[:-1]) // 512) % 2)[None, :], len(ars) - 1, axis=0)
    c_own = np.repeat((np.array(crs[:-1]) // 1024)[:, None], len(ccs) - 1, axis=1)
    a_case, c_case = Custom(ars, acs, a_own, ord="C"), Custom(crs, ccs, c_own, ord="C", ld_pad=1)
    a = [oracle.gen(dt, 0x81, r, a_case.buf_elems(r, P)) for r in range(P)]
    c = [oracle.gen(dt, 0x82, r, c_case.buf_elems(r, P)) for r in range(P)]
    exp = [x.copy() for x in c]
    oracle.transform(dt, "C", alpha, beta, a_case.geom(P), a, c_case.geom(P), exp)
    assert all(np.isfinite(x).all() for x in exp)
    da, dc = [dev(x) for x in a], [dev(x) for x in c]
    lay = [(a_case.make_layout(r, da[r].data_ptr(), P, dt), c_case.make_layout(r, dc[r].data_ptr(), P, dt))
           for r in range(P)]
    plans = [gpu.plan_export([A], [C], r, P, ["C"], [alpha], [beta]) for r, (A, C) in enumerate(lay)]
    for r, p in enumerate(plans):
        q = 1 - r
        assert int(p.send_counts[q]) * 16 == 16 << 20 and int(p.recv_counts[q]) * 16 == 16 << 20
        assert pair_parts(gpu, int(p.send_counts[q]), 16, 4) == 4
        assert [gpu.round_range(int(p.send_counts[q]), 16, 4, k)[0] for k in range(4)] == \
            [k << 18 for k in range(4)]
        assert p.local_ops.size > 0
        # all three cuts of the pair, on both sides
        assert _straddled(gpu, p.pack_ops, "dst", p.send_displs, p.send_counts, r, 16, 4) == 3
        assert _straddled(gpu, p.unpack_ops, "src", p.recv_displs, p.recv_counts, r, 16, 4) == 3

    def call(r, comm):
        gpu.transform(lay[r][0], lay[r][1], comm, "C", alpha, beta)

    out = drive(gpu, plans, 16, call)
    assert out.multi_pairs == 2 and out.max_parts == 4
    assert out.stats["pack_launches"] == 8 and out.stats["unpack_launches"] == 8, out.stats
    for r in range(P):
        got = host(dc[r], np.complex128)
        bad = np.flatnonzero(got.view(np.uint64) != exp[r].view(np.uint64))
        assert bad.size == 0, f"rank {r}: {bad.size} words differ, first at element {bad[0] // 2}"


# ------------------------------------------------------------------ d. family cases (child process)
@pytest.mark.parametrize("family", list(FAMILY_CASES))
def test_family_on_four_ranks(family):
    """tests/emulated_family_child.py with the round threshold at 2048 bytes (read once per process):
    every family's transforms on 4 emulated ranks, 4 rounds, against the global oracle"""
    child = os.path.join(HERE, "emulated_family_child.py")
    env = dict(os.environ, COSTA_TUNING="1", COSTA_ROUND_MIN_BYTES="2048")
    r = subprocess.run([sys.executable, child, family], env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1].startswith("OK"), r.stdout + r.stderr
    _, n, multi = out[-1].split()
    assert int(n) == FAMILY_CASES[family], out[-1]
    assert int(multi) >= int(n), out[-1]  # at least one multi-round pair per case


# ------------------------------------------------------------------ e. refusals
def _small(gpu, on_device=True):
    a, c = np.zeros(64 * 64), np.zeros(64 * 64)
    keep = (dev(a), dev(c)) if on_device else (a, c)
    pa, pc = (x.data_ptr() if on_device else x for x in keep)
    mk = gpu.block_cyclic_layout
    return (mk(64, 64, 32, 32, 1, 1, 64, 64, 1, 2, "R", 0, 0, pa, 64, "C", 0),
            mk(64, 64, 32, 32, 1, 1, 64, 64, 2, 1, "R", 0, 0, pc, 64, "C", 0), keep)


def test_refuses_without_a_part(gpu):
    A, C, _ = _small(gpu)
    comm = gpu.Comm.emulated(0, 2, 0)
    assert (comm.rank, comm.size) == (0, 2)
    with pytest.raises(gpu.CostaError, match="no part selected") as e:
        gpu.transform(A, C, comm, "N", 1.0, 0.0)
    assert e.value.code == 1


def test_refuses_host_layouts(gpu):
    A, C, _ = _small(gpu, on_device=False)
    comm = gpu.Comm.emulated(0, 2, 0)
    comm.emulate("local")
    with pytest.raises(gpu.CostaError, match="emulated communicator needs device-resident") as e:
        gpu.transform(A, C, comm, "N", 1.0, 0.0)
    assert e.value.code == 1


def test_refuses_async(gpu):
    A, C, _ = _small(gpu)
    comm = gpu.Comm.emulated(0, 2, 0)
    comm.emulate("local")
    with pytest.raises(gpu.CostaError, match="blocking transforms only") as e:
        gpu.transform_async(A, C, comm, "N", 1.0, 0.0)
    assert e.value.code == 1


def test_refuses_a_real_communicator(gpu):
    with pytest.raises(gpu.CostaError, match="not an emulated communicator") as e:
        gpu.Comm.self(0).emulate("local")
    assert e.value.code == 1


def test_refuses_bad_selections(gpu):
    comm = gpu.Comm.emulated(1, 2, 0)
    pkg = poisoned(4096)
    with pytest.raises(gpu.CostaError, match="not aligned to 256"):
        comm.emulate("pack", 0, pkg.data_ptr() + 64)
    with pytest.raises(gpu.CostaError, match="not a device pointer"):
        comm.emulate("unpack", 0, np.zeros(512))
    with pytest.raises(gpu.CostaError, match="not a device pointer"):
        comm.emulate("pack", 0, None)
    with pytest.raises(gpu.CostaError, match="not PACK, UNPACK or LOCAL"):
        comm.emulate(7, 0, pkg)
    for rnd in (-2, gpu.exchange_rounds()):
        with pytest.raises(gpu.CostaError, match="round"):
            comm.emulate("pack", rnd, pkg)
    with pytest.raises(gpu.CostaError, match="bad rank/size"):
        gpu.Comm.emulated(2, 2, 0)


def test_refuses_a_short_package(gpu):
    """a package whose device allocation cannot hold the plan's send elements is refused before any
    launch: 8 MiB to send, and a 4 KiB tensor, which torch carves out of a 2 MiB allocation"""
    n = 2048
    da = torch.zeros(n * n, dtype=torch.float64, device="cuda")
    dc = torch.zeros(n * n, dtype=torch.float64, device="cuda")
    mk = gpu.block_cyclic_layout
    A = mk(n, n, 128, 128, 1, 1, n, n, 1, 2, "R", 0, 0, da.data_ptr(), n, "C", 0)
    C = mk(n, n, 128, 128, 1, 1, n, n, 2, 1, "R", 0, 0, dc.data_ptr(), n // 2, "C", 0)
    plan = gpu.plan_export([A], [C], 0, 2, ["N"], [1.0], [0.0])
    assert plan.send_elems * 8 == 8 << 20
    comm = gpu.Comm.emulated(0, 2, 0)
    comm.emulate("pack", 0, poisoned(4096))
    with pytest.raises(gpu.CostaError, match="smaller than the plan's"):
        gpu.transform(A, C, comm, "N", 1.0, 0.0)
    assert bool((dc == 0).all())
