"""Shared model of triangular (masked) transforms for test_tri_plan_cpu.py and test_gpu_tri.py.

The plans of every rank come from costa_amd.plan_export_tri.  On the CPU the ordinary ops run
through the oracle's copy_and_transform, each edge op runs through it too and the dropped elements
of its destination are put back afterwards, and the exchange is simulated by slicing.  The expected
result is where(mask, C_full, C_before) on every rank's buffer, C_full being the ordinary plan
(costa_amd.plan_export) run through the oracle.
"""
import numpy as np

import oracle
from casegen import BC, Custom

UPLOS = ("U", "L")
KS = (0, 1, -1, -64, 10000, -10000)
SCALARS = {oracle.DOUBLE: (0.75, -1.5), oracle.CFLOAT: (0.75 - 0.5j, 1.25 + 0.25j),
           oracle.CDOUBLE: (0.75 - 0.5j, 1.25 + 0.25j), oracle.FLOAT: (0.75, -1.5),
           oracle.INT32: (3, -2)}


def keep_mask(m, n, uplo, k):
    """keep(i, j) of an m x n target: numpy triu(k) / tril(k)"""
    d = np.arange(n)[None, :] - np.arange(m)[:, None]
    return d >= k if uplo.upper() == "U" else d <= k


def distribute(dense, case, P):
    """per-rank float64 buffers of `case` holding the dense matrix (0 in the padding)"""
    m, n = dense.shape
    src = Custom([0, m], [0, n], [[0]], ord="C")
    a = [np.asfortranarray(dense, np.float64).reshape(-1, order="F").copy()]
    a += [np.zeros(1) for _ in range(P - 1)]
    out = [np.zeros(case.buf_elems(r, P)) for r in range(P)]
    oracle.transform(oracle.DOUBLE, "N", 1, 0, src.geom(P), a, case.geom(P), out)
    return out


def cases_geometry(shape, grid, op):
    """(A case, C case) of the block-cyclic test geometry: blocks (32, 48) -> (40, 24)"""
    m, n = shape
    pm, pn = grid
    am, an = (n, m) if op != "N" else (m, n)
    return BC(am, an, 32, 48, pm=pm, pn=pn), BC(m, n, 40, 24, pm=pm, pn=pn)


def inputs(dtype, a_case, c_case, P, seed=7):
    return [(oracle.gen(dtype, seed, r, a_case.buf_elems(r, P)),
             oracle.gen(dtype, seed + 100, r, c_case.buf_elems(r, P))) for r in range(P)]


def poison_dropped(bufs, a_case, c_case, P, op, uplo, k):
    """NaN at every element of A that maps to a dropped target position (and in A's padding)"""
    m, n = c_case.shape()
    keep = keep_mask(m, n, uplo, k).astype(np.float64)
    ka = distribute(keep.T.copy() if op != "N" else keep, a_case, P)
    for r in range(P):
        bufs[r][0][ka[r] == 0] = np.nan


def kept_of_op(t):
    """(destination element offsets, kept) of one edge op, both nf x ns in (f, s)"""
    nf, ns, ldd, flags, d = (int(t[x]) for x in ("nf", "ns", "ldd", "flags", "diag"))
    f, s = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
    off = f * ldd + s if flags & 1 else s * ldd + f
    kept = (s - f <= d) if flags & 0x40 else (s - f >= d)
    return off, kept


def as_tile_ops(costa, tri):
    ops = np.zeros(tri.size, costa.TILE_OP_DTYPE)
    for name in costa.TILE_OP_DTYPE.names:
        ops[name] = tri[name]
    ops["flags"] &= ~np.uint32(0x40)
    return ops


def oracle_edge_ops(costa, dtype, tri, scalars, dst_buf, src_base=0, exec_ops=oracle.exec_tile_ops):
    """edge ops on host memory: the whole op through the oracle, then the dropped elements of the
    destination (absolute addresses inside dst_buf) are restored, bit for bit; exec_ops: the
    executor of one op (specials_common.exec_ops for lists with op forms no plan holds)"""
    E = dst_buf.itemsize
    raw = dst_buf.view(f"V{E}")
    ops = as_tile_ops(costa, tri)
    for t, op in zip(tri, ops):
        off, kept = kept_of_op(t)
        assert (int(t["dst"]) - dst_buf.ctypes.data) % E == 0
        idx = (int(t["dst"]) - dst_buf.ctypes.data) // E + off
        assert idx.min() >= 0 and idx.max() < dst_buf.size
        old = raw[idx[~kept]].copy()
        exec_ops(dtype, op.reshape(1), scalars, src_base, 0)
        raw[idx[~kept]] = old


def make_plans(costa, dtype, a_case, c_case, P, bufs, op, alpha, beta, uplo=None, k=0):
    """every rank's plan on the given buffers; uplo None: the ordinary plan"""
    plans, keep = [], []
    for r in range(P):
        A = a_case.make_layout(r, bufs[r][0].ctypes.data, P, dtype)
        C = c_case.make_layout(r, bufs[r][1].ctypes.data, P, dtype)
        keep.append((A, C))
        if uplo is None:
            plans.append(costa.plan_export([A], [C], r, P, [op], [alpha], [beta]))
        else:
            plans.append(costa.plan_export_tri(A, C, r, P, op, uplo, k, alpha, beta))
    return plans, keep


def run_plans_cpu(costa, dtype, plans, bufs):
    """PACK, the exchange by slicing, UNPACK and LOCAL (ordinary and edge lists) on the host"""
    P = len(plans)
    npd = oracle.NP[dtype]
    send = [np.zeros(max(1, p.send_elems), npd) for p in plans]
    recv = [np.zeros(max(1, p.recv_elems), npd) for p in plans]
    for r, p in enumerate(plans):
        oracle.exec_tile_ops(dtype, p.pack_ops, p.scalars, 0, send[r].ctypes.data)
        assert p.send_counts.sum() == p.send_elems and p.recv_counts.sum() == p.recv_elems
    for r in range(P):
        for q in range(P):
            n = plans[r].recv_counts[q]
            assert n == plans[q].send_counts[r]
            d, s = plans[r].recv_displs[q], plans[q].send_displs[r]
            recv[r][d:d + n] = send[q][s:s + n]
    for r, p in enumerate(plans):
        oracle.exec_tile_ops(dtype, p.unpack_ops, p.scalars, recv[r].ctypes.data, 0)
        oracle.exec_tile_ops(dtype, p.local_ops, p.scalars, 0, 0)
        if getattr(p, "unpack_tri", None) is not None:
            oracle_edge_ops(costa, dtype, p.unpack_tri, p.scalars, bufs[r][1], recv[r].ctypes.data)
            oracle_edge_ops(costa, dtype, p.local_tri, p.scalars, bufs[r][1])


class Reference:
    """C_before and C_full (the ordinary plan through the oracle) of one geometry, computed once"""

    def __init__(self, costa, dtype, a_case, c_case, P, op, alpha, beta, seed=7):
        self.dtype, self.a_case, self.c_case, self.P, self.op = dtype, a_case, c_case, P, op
        self.alpha, self.beta, self.seed = alpha, beta, seed
        bufs = inputs(dtype, a_case, c_case, P, seed)
        self.before = [c.copy() for _, c in bufs]
        plans, keep = make_plans(costa, dtype, a_case, c_case, P, bufs, op, alpha, beta)
        run_plans_cpu(costa, dtype, plans, bufs)
        self.full = [c for _, c in bufs]
        self.full_plans = plans
        self.shape = c_case.shape()

    def fresh(self):
        return inputs(self.dtype, self.a_case, self.c_case, self.P, self.seed)

    def expected(self, uplo, k):
        m, n = self.shape
        kc = distribute(keep_mask(m, n, uplo, k).astype(np.float64), self.c_case, self.P)
        return [np.where(kc[r] == 1, self.full[r], self.before[r]) for r in range(self.P)]


def same_bytes(a, b):
    return a.tobytes() == b.tobytes()
