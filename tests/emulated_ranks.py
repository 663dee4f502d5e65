"""P ranks of an N > 1 transform on ONE GPU, through the code a real multi-rank transform() runs.

Every rank gets an emulated communicator (costa_amd.Comm.emulated): its plans, exchange rounds and
pack / unpack work lists are those of an RCCL communicator of that rank and size, and
``comm.emulate(part, round, buffer)`` makes the next transform call launch one part of it against
the caller's package.  The driver below is the exchange: per round it copies, for every ordered pair
of ranks, exactly the element range ``costa_amd.round_range`` gives (what issue_exchange would hand
to ncclSend / ncclRecv) from the sender's package to the receiver's.  Both packages start as 0xFF
bytes, a NaN in every floating type here (e4m3 included), and arrivals are staged round by round over
that poison: a pack op in too late a round, an unpack op in too early a round or a segment that was
never packed shows as a NaN or a byte mismatch in the destination, provided the expected values
are finite.

Shared by tests/test_gpu_emulated_ranks.py and tests/emulated_family_child.py.
"""
from dataclasses import dataclass

import numpy as np

PKG_ALIGN = 256


def dev(arr):
    """device copy of a numpy buffer (raw bytes, any dtype)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def poisoned(nbytes):
    """a device package of 0xFF bytes, aligned as the library's own packages are"""
    import torch
    t = torch.full((max(1, int(nbytes)),), 0xFF, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % PKG_ALIGN == 0
    return t


def pair_parts(costa, count, esize, rounds):
    """how many rounds move a non-empty part of a pair's package of `count` elements"""
    n = 0
    for r in range(rounds):
        lo, hi = costa.round_range(count, esize, rounds, r)
        n += hi > lo
    return n


def check_geometry(plans):
    """the exchange geometry of every rank's exported plan is consistent: what p receives from q is
    what q sends to p, and every pair's segment lies inside its package"""
    P = len(plans)
    for p in range(P):
        pl = plans[p]
        assert int(pl.send_counts.sum()) == pl.send_elems and int(pl.recv_counts.sum()) == pl.recv_elems
        for q in range(P):
            assert int(pl.recv_counts[q]) == int(plans[q].send_counts[p]), (p, q)
            assert 0 <= int(pl.send_displs[q]) and int(pl.send_displs[q] + pl.send_counts[q]) <= pl.send_elems
            assert 0 <= int(pl.recv_displs[q]) and int(pl.recv_displs[q] + pl.recv_counts[q]) <= pl.recv_elems


@dataclass
class Outcome:
    rounds: int        # exchange rounds of the process
    multi_pairs: int   # off-rank pairs whose package moved in more than one part
    max_parts: int     # the most parts any off-rank pair moved in
    stats: dict        # get_stats() deltas over the whole run


def drive(costa, plans, esize, call, local_first=False, device=0):
    """Run the transform `call(rank, comm)` of every rank through PACK(r) -> exchange(r) -> UNPACK(r)
    for every round r, and LOCAL once per rank (before the loop or after it).

    plans  every rank's exported plan (only its exchange geometry is used: counts, displacements)
    esize  bytes of a package element
    call   issues rank's transform on its emulated communicator; called once per part and round
    """
    import torch
    P = len(plans)
    check_geometry(plans)
    R = costa.exchange_rounds()
    comms = [costa.Comm.emulated(r, P, device) for r in range(P)]
    send = [poisoned(p.send_elems * esize) for p in plans]
    recv = [poisoned(p.recv_elems * esize) for p in plans]
    st0 = costa.get_stats()

    def part(name, r=-1):
        for q in range(P):
            buf = {"pack": send[q], "unpack": recv[q], "local": None}[name]
            comms[q].emulate(name, r, buf)
            call(q, comms[q])

    if local_first:
        part("local")
    parts = {}
    for r in range(R):
        part("pack", r)
        for p in range(P):
            for q in range(P):
                n = int(plans[p].recv_counts[q])
                lo, hi = costa.round_range(n, esize, R, r)
                assert 0 <= lo <= hi <= n
                if hi > lo:
                    parts[(p, q)] = parts.get((p, q), 0) + 1
                    s = (int(plans[q].send_displs[p]) + lo) * esize
                    d = (int(plans[p].recv_displs[q]) + lo) * esize
                    nb = (hi - lo) * esize
                    assert s + nb <= send[q].numel() and d + nb <= recv[p].numel()
                    recv[p][d:d + nb].copy_(send[q][s:s + nb])
        torch.cuda.synchronize()
        part("unpack", r)
    if not local_first:
        part("local")
    st = costa.get_stats()
    for c in comms:
        c.close()
    off = [v for (p, q), v in parts.items() if p != q]
    return Outcome(R, sum(1 for v in off if v > 1), max(off, default=0),
                   {k: st[k] - st0[k] for k in st if isinstance(st[k], int)})


# ------------------------------------------------------------------ the plan's byte counts
def alg_bytes(ops, src_elem, dst_elem):
    """algorithmic bytes of a tile-op list, each side at its own element size (the planner's rule:
    the source is read unless the op stores zeros, the destination is written, and read too by
    beta*C + alpha*op(A) ops)"""
    if ops.size == 0:
        return 0
    kind = (ops["flags"].astype(np.int64) >> 4) & 3
    n = ops["nf"].astype(np.int64) * ops["ns"].astype(np.int64)
    return int((src_elem * n * (kind != 1) + dst_elem * n * (1 + (kind == 3))).sum())
