"""Child process of test_gpu_emulated_ranks.py: one family of transforms ('plain', 'half', 'fp8',
'tri', 'scaled' or 'amax', the first argument) on P = 4 emulated ranks of one GPU, with exchange
rounds at fixture size (the parent sets COSTA_TUNING=1 COSTA_ROUND_MIN_BYTES=2048; the threshold is
read once per process).  Geometries 'bc203' and 'cfg5' of half_common.geometry on a 2 x 2 grid, ops
'N' and 'T' ('C' for complex pairs), alpha = -0.5, beta = 2.

Each rank's transform runs through tests/emulated_ranks.drive: the product's per-round pack and
unpack lists against poisoned packages.  The expected C of every rank is the family's existing recipe
(*_common.expected_transform) generalised from geom(1) to geom(P): the global oracle.transform over
all ranks' buffers (tri: tri_common.Reference).  Whole destination buffers are compared byte for
byte, so padding and gaps must keep their fill.  Every case asserts that each rank sends, receives
and has a LOCAL list, and that some off-rank pair of at least 2048 bytes moved in 4 parts.

'--dry' builds the cases, plans and expected values on the host only (no GPU) and checks the
coverage conditions.  Stops at the first failure ('FAIL ...', exit status 1) and starts nothing more
on the GPU; else prints 'OK <cases> <multi-round pairs>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import costa_amd as costa  # noqa: E402
import fp8_common as fc  # noqa: E402
import half_common as hc  # noqa: E402
import oracle  # noqa: E402
import scaled_common as sc  # noqa: E402
from amax_common import _reduce_layout, assert_moved, assert_vec, layout_index, matrix_data  # noqa: E402
from casegen import Custom  # noqa: E402
from emulated_ranks import dev, drive, pair_parts  # noqa: E402
from scaled_common import BF16, D, E4M3, E5M2, F, H16  # noqa: E402
from tri_common import Reference  # noqa: E402

P, GRID = 4, (2, 2)
ALPHA, BETA = -0.5, 2.0
GEOMS = ("bc203", "cfg5")
MIN_BYTES = 2048
CF = oracle.CFLOAT
NAMES = {**sc.NAMES, CF: "c64"}
ESIZE = dict(sc.ESIZE)
NPT = {**sc.NPT, CF: np.complex64}

FAMILIES = {
    "plain": [(D, D), (CF, CF), (D, F), (F, D)],
    "half": [(F, BF16), (H16, F), (BF16, BF16)],
    "fp8": [(F, E4M3), (E4M3, F), (E5M2, E5M2)],
    "tri": [(D, "U", 0), (CF, "L", -3)],
    "scaled": [(F, F), (F, E4M3), (E4M3, F), (BF16, BF16), (D, D)],
    "amax": [(F, E4M3), (BF16, BF16)],
}


def fail(msg):
    print("FAIL", msg)
    sys.exit(1)


def pkg_code(ta, tc):
    """element type of the packages: A's for FP8 pairs, else the narrower of the two"""
    if ta in (E4M3, E5M2) or tc in (E4M3, E5M2):
        return ta
    return ta if ESIZE[ta] <= ESIZE[tc] else tc


def family_cases(family):
    """(name, pair or tri spec, geometry, op, vectors) of every case of a family"""
    out = []
    for spec in FAMILIES[family]:
        cplx = spec[0] == CF
        for g in GEOMS:
            for op in ("N", "C" if cplx else "T"):
                if family == "tri":
                    name = f"tri {NAMES[spec[0]]} {spec[1]} k={spec[2]} {g} {op}"
                else:
                    name = f"{family} {NAMES[spec[0]]}->{NAMES[spec[1]]} {g} {op}"
                out.append((name, spec, g, op, "rc"))
    if family == "scaled":  # one case with a column vector only
        out.append(("scaled f32->f32 bc203 T col-only", (F, F), "bc203", "T", "c"))
    return out


def gen_all(code, seed, case):
    """every rank's buffer of `case`, each from its own stream"""
    if code in (D, CF):
        return [oracle.gen(code, seed, r, case.buf_elems(r, P)) for r in range(P)]
    return [sc.gen(code, seed + 16 * r, case.buf_elems(r, P)) for r in range(P)]


def source_values(a, ta, tc, family):
    """A's buffers as the pair delivers them to its arithmetic, in the oracle's type"""
    if family == "plain":
        return [x.astype(oracle.NP[tc]) for x in a]
    if family == "half":
        return [hc.widen(hc.cvt(hc.widen(x, ta), tc) if ta == F else x, tc if ta == F else ta) for x in a]
    if family == "fp8":
        return [fc.widen(x, ta) for x in a]
    return [sc.source_values(x, ta, tc) for x in a]


def dense_of(oc, ct, op, a_case, wa, m, n):
    """op(A) gathered into one m x n matrix (an exact redistribution by the oracle)"""
    whole = Custom([0, m], [0, n], [[0]], ord="C")
    out = [np.zeros(whole.buf_elems(r, P), ct) for r in range(P)]
    oracle.transform(oc, op, 1, 0, a_case.geom(P), wa, whole.geom(P), out)
    return out[0].reshape(m, n, order="F")


class Built:
    """one case on the host: inputs, expected values and every rank's plan"""

    def __init__(self, family, spec, geom, op, vectors):
        self.family, self.op = family, op
        self.a_case, self.c_case = a_case, c_case = sc.geometry(geom, op, grid=GRID)
        self.r = self.cs = self.r0 = self.c0 = self.exp_r = self.exp_c = None
        if family == "tri":
            dt, self.uplo, self.k = spec
            self.ta = self.tc = dt
            self.ref = Reference(costa, dt, a_case, c_case, P, op, ALPHA, BETA)
            bufs = self.ref.fresh()
            self.a, self.c = [b[0] for b in bufs], [b[1] for b in bufs]
            self.exp = self.ref.expected(self.uplo, self.k)
        else:
            self.ta, self.tc = ta, tc = spec
            if family == "amax":
                self.a = [matrix_data(ta, 0x71, a_case, P, r) for r in range(P)]
            else:
                self.a = gen_all(ta, 0x71, a_case)
            self.c = gen_all(tc, 0x72, c_case)
            wa = source_values(self.a, ta, tc, family)
            if family in ("plain", "half", "fp8"):
                oc = tc if family == "plain" else oracle.FLOAT
                wc = [x.copy() for x in self.c] if family == "plain" else [sc.widen(x, tc) for x in self.c]
                oracle.transform(oc, op, ALPHA, BETA, a_case.geom(P), wa, c_case.geom(P), wc)
                self.exp = wc if family == "plain" else [sc.cvt(x, tc) for x in wc]
            else:
                self._scaled(wa, vectors)
        self.esize = ESIZE[pkg_code(self.ta, self.tc)]

    def _scaled(self, wa, vectors):
        """scaled_common.expected_transform over P ranks, the row / column of every buffer element
        from amax_common.layout_index; for amax also every rank's expected vectors"""
        ta, tc, op, a_case, c_case = self.ta, self.tc, self.op, self.a_case, self.c_case
        ct, oc = sc.ctype(ta, tc), sc.ocode(ta, tc)
        m, n = c_case.shape()
        self.r = sc.scales(m, 0x73, ct) if "r" in vectors else None
        self.cs = sc.scales(n, 0x74, ct) if "c" in vectors else None
        T = [np.zeros(c_case.buf_elems(r, P), ct) for r in range(P)]
        oracle.transform(oc, op, 1, 0, a_case.geom(P), wa, c_case.geom(P), T)
        idx = layout_index(c_case, P)
        X = []
        for r in range(P):
            ii, jj, _, _ = idx[r]
            x = T[r]
            if self.r is not None:
                x = x * self.r[ii]
            if self.cs is not None:
                x = x * self.cs[jj]
            assert x.dtype == ct
            X.append(np.ascontiguousarray(x))
        wc = [sc.widen(x, tc).astype(ct) for x in self.c]
        oracle.transform(oc, "N", ALPHA, BETA, c_case.geom(P), X, c_case.geom(P), wc)
        self.exp = [sc.cvt(x, tc) for x in wc]
        if self.family != "amax":
            return
        self.r0, self.c0 = np.zeros(m, ct), np.zeros(n, ct)
        vec = [_reduce_layout(T[r], c_case, P, r, self.r0, self.c0) for r in range(P)]
        self.exp_r, self.exp_c = [v[0] for v in vec], [v[1] for v in vec]
        # each rank's vectors hold its own part of C: their maximum over ranks is the dense amax
        dense = np.abs(dense_of(oc, ct, op, a_case, wa, m, n))
        assert np.array_equal(np.maximum.reduce(self.exp_r), dense.max(axis=1))
        assert np.array_equal(np.maximum.reduce(self.exp_c), dense.max(axis=0))
        for r in range(P):
            assert_moved(self.exp_r[r], self.r0, f"rank {r} row_amax")
            assert_moved(self.exp_c[r], self.c0, f"rank {r} col_amax")

    def layouts(self, rank, pa, pc):
        return (sc.make_layout(costa, self.a_case, rank, pa, P, self.ta),
                sc.make_layout(costa, self.c_case, rank, pc, P, self.tc))

    def plan(self, rank, A, C):
        if self.family == "tri":
            return costa.plan_export_tri(A, C, rank, P, self.op, self.uplo, self.k, ALPHA, BETA)
        if self.family in ("scaled", "amax"):
            return costa.plan_export_scaled(A, C, rank, P, self.op, ALPHA, BETA)
        return costa.plan_export([A], [C], rank, P, [self.op], [ALPHA], [BETA])

    def assert_finite(self, what):
        for r in range(P):
            if self.tc in (D, CF):
                assert np.isfinite(self.exp[r]).all(), f"{what}: the expected buffer holds a NaN or an inf"
            else:
                sc.assert_finite(self.exp[r], self.tc, what)


def coverage(name, plans, esize, rounds):
    """every rank sends, receives and has a LOCAL list; some off-rank pair of at least MIN_BYTES
    gets `rounds` parts.  Returns the number of such pairs."""
    multi = 0
    for r, p in enumerate(plans):
        n_local = p.local_ops.size + getattr(p, "local_tri", np.zeros(0)).size + \
            getattr(p, "local_scaled", np.zeros(0)).size
        if not (p.send_elems > 0 and p.recv_elems > 0 and n_local > 0):
            fail(f"{name}: rank {r} sends {p.send_elems}, receives {p.recv_elems}, {n_local} local ops")
        for q in range(P):
            n = int(p.send_counts[q])
            if q != r and n * esize >= MIN_BYTES:
                if pair_parts(costa, n, esize, rounds) != rounds:
                    fail(f"{name}: the {n * esize}-byte package {r} -> {q} is not in {rounds} parts")
                multi += 1
    if rounds != 4 or multi == 0:
        fail(f"{name}: {rounds} rounds, {multi} off-rank pairs of at least {MIN_BYTES} bytes")
    return multi


def run_case(k, name, b, dry):
    b.assert_finite(name)
    R = costa.exchange_rounds()
    if dry:
        keep = [b.layouts(r, b.a[r].ctypes.data, b.c[r].ctypes.data) for r in range(P)]
        plans = [b.plan(r, *keep[r]) for r in range(P)]
        return coverage(name, plans, b.esize, R)
    import torch
    da, dc = [dev(x) for x in b.a], [dev(x) for x in b.c]
    lay = [b.layouts(r, da[r].data_ptr(), dc[r].data_ptr()) for r in range(P)]
    plans = [b.plan(r, *lay[r]) for r in range(P)]
    multi = coverage(name, plans, b.esize, R)
    vec = {}
    if b.family in ("scaled", "amax"):
        vec["row_scale"] = None if b.r is None else torch.from_numpy(b.r).cuda()
        vec["col_scale"] = None if b.cs is None else torch.from_numpy(b.cs).cuda()
    ra = [torch.from_numpy(b.r0).cuda() for _ in range(P)] if b.family == "amax" else None
    ca = [torch.from_numpy(b.c0).cuda() for _ in range(P)] if b.family == "amax" else None

    def call(r, comm):
        A, C = lay[r]
        if b.family == "tri":
            costa.transform_tri(A, C, comm, b.op, b.uplo, b.k, ALPHA, BETA)
        elif b.family == "scaled":
            costa.transform_scaled(A, C, comm, b.op, ALPHA, BETA, **vec)
        elif b.family == "amax":
            costa.transform_amax(A, C, comm, b.op, ALPHA, BETA, row_amax=ra[r], col_amax=ca[r], **vec)
        else:
            costa.transform(A, C, comm, b.op, ALPHA, BETA)

    out = drive(costa, plans, b.esize, call, local_first=k % 2 == 1)
    if out.multi_pairs != multi or out.max_parts != R:
        fail(f"{name}: {out.multi_pairs} pairs moved in several parts ({multi} expected), at most "
             f"{out.max_parts} parts")
    if out.stats["pack_launches"] <= 0 or out.stats["unpack_launches"] <= 0:
        fail(f"{name}: no pack or no unpack launch")
    try:
        for r in range(P):
            got = dc[r].cpu().numpy().view(NPT[b.tc])
            if b.tc in (D, CF):
                assert got.tobytes() == b.exp[r].tobytes(), \
                    f"{name}: rank {r}: C differs from the oracle at element " \
                    f"{np.flatnonzero(got.view(np.uint8) != b.exp[r].view(np.uint8))[:1] // got.itemsize}"
            else:
                sc.assert_bits(got, b.exp[r], b.tc, f"{name}: rank {r}")
            if b.family == "amax":
                assert_vec(ra[r].cpu().numpy(), b.exp_r[r], f"{name}: rank {r} row_amax")
                assert_vec(ca[r].cpu().numpy(), b.exp_c[r], f"{name}: rank {r} col_amax")
    except AssertionError as e:
        fail(str(e))
    return multi


def main():
    family = sys.argv[1]
    dry = "--dry" in sys.argv[2:]
    assert family in FAMILIES
    if costa.round_range(MIN_BYTES, 1, 4, 1) == (MIN_BYTES, MIN_BYTES):
        fail(f"a {MIN_BYTES}-byte package is one part: COSTA_TUNING=1 COSTA_ROUND_MIN_BYTES={MIN_BYTES} not set")
    n = multi = 0
    for k, (name, spec, geom, op, vectors) in enumerate(family_cases(family)):
        multi += run_case(k, name, Built(family, spec, geom, op, vectors), dry)
        n += 1
    print("OK", n, multi)
    return 0


if __name__ == "__main__":
    sys.exit(main())
