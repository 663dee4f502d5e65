"""Child process of test_gpu_mixed.py (run with COSTA_LOOPBACK=1 or 2): mixed-precision
transforms of the 203 x 157 block-cyclic case, fp64 -> fp32 and fp32 -> fp64, 'N' and 'T' with
alpha, beta, go through PACK -> ncclSend/ncclRecv to self -> UNPACK (mode 2: half of the tiles,
the rest through the concurrent LOCAL launch).  The package holds the narrower type: narrowing
pairs convert while packing, widening pairs while unpacking.  Each result is compared bit for bit
with the CPU oracle run in C's type on the converted A, and the algorithmic byte counts of the
pack and unpack lists with what a package of the narrower type gives.  Stops at the first failure
('FAIL ...', exit status 1); else prints 'OK <cases> <pack> <unpack> <local launches>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
import oracle  # noqa: E402
from casegen import BC  # noqa: E402

M, N = 203, 157
ESIZE = {oracle.FLOAT: 4, oracle.DOUBLE: 8}


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def fail(msg):
    print("FAIL", msg)
    sys.exit(1)


def main():
    mode = os.environ.get("COSTA_LOOPBACK")
    assert mode in ("1", "2")
    comm = costa.Comm.self(0)
    costa.get_stats(reset=True)
    n = 0
    for ta, tc in ((oracle.DOUBLE, oracle.FLOAT), (oracle.FLOAT, oracle.DOUBLE)):
        for op, alpha, beta in (("N", 1, 0), ("T", -0.5, 2.0)):
            what = f"{ta}->{tc} {op}"
            am, an = (N, M) if op == "T" else (M, N)
            a_case, c_case = BC(am, an, 32, 48), BC(M, N, 40, 24)
            a = oracle.gen(ta, 0x71, 0, a_case.buf_elems(0, 1))
            c = oracle.gen(tc, 0x72, 0, c_case.buf_elems(0, 1))
            exp = c.copy()
            oracle.transform(tc, op, alpha, beta, a_case.geom(1), [a.astype(oracle.NP[tc])],
                             c_case.geom(1), [exp])
            da, dc = dev(a), dev(c)
            st0 = costa.get_stats()
            costa.transform(a_case.make_layout(0, da.data_ptr(), 1, ta),
                            c_case.make_layout(0, dc.data_ptr(), 1, tc), comm, op, alpha, beta)
            st = costa.get_stats()
            if dc.cpu().numpy().tobytes() != exp.tobytes():
                fail(f"{what}: result differs from the oracle")
            if st["pack_launches"] == st0["pack_launches"] or st["unpack_launches"] == st0["unpack_launches"]:
                fail(f"{what}: no pack or no unpack launch")
            # the package holds the narrower type: pack moves E_A + E_P bytes per element, unpack
            # E_P + E_C (+ E_C when beta != 0)
            ea, ec = ESIZE[ta], ESIZE[tc]
            ep = min(ea, ec)
            pb = st["pack_bytes"] - st0["pack_bytes"]
            ub = st["unpack_bytes"] - st0["unpack_bytes"]
            if pb <= 0 or pb % (ea + ep):
                fail(f"{what}: pack_bytes {pb} is no multiple of {ea + ep}")
            moved = pb // (ea + ep)
            if mode == "1" and moved != M * N:
                fail(f"{what}: {moved} elements packed, {M * N} expected")
            if mode == "2" and not 0 < moved < M * N:
                fail(f"{what}: {moved} elements packed of {M * N}")
            if ub != moved * (ep + ec * (2 if beta else 1)):
                fail(f"{what}: unpack_bytes {ub} for {moved} elements")
            if st["convert_items"] == st0["convert_items"]:
                fail(f"{what}: no converting sub-tile ran")
            n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
