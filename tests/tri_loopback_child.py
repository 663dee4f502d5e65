"""Child process of test_gpu_tri.py (run with COSTA_LOOPBACK=1 or 2): triangular transforms of the
200 x 136 block-cyclic case and of a single block cut into bands go through PACK -> ncclSend/ncclRecv
to self -> UNPACK (mode 2: half of the tiles, the rest through the concurrent LOCAL launch), edge
tiles included, and so does the in-place fill of a triangle.  Each result is compared bit for bit
with where(mask, C_full, C_before) from the CPU oracle.  Stops at the first failure ('FAIL ...',
exit status 1); else prints 'OK <cases> <pack launches> <unpack launches> <tri_items>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
import oracle  # noqa: E402
from casegen import BC, Custom  # noqa: E402
from tri_common import SCALARS, Reference, cases_geometry, keep_mask  # noqa: E402


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
    side = 2 * costa.tri_cut() + 37
    geoms = [(oracle.DOUBLE, "N", *cases_geometry((200, 136), (1, 1), "N")),
             (oracle.DOUBLE, "T", *cases_geometry((200, 136), (1, 1), "T")),
             (oracle.CFLOAT, "C", *cases_geometry((136, 200), (1, 1), "C")),
             (oracle.DOUBLE, "T", Custom([0, side], [0, side], [[0]], ord="C"),
              Custom([0, side], [0, side], [[0]], ord="R"))]
    for dtype, op, a_case, c_case in geoms:
        alpha, beta = SCALARS[dtype]
        ref = Reference(costa, dtype, a_case, c_case, 1, op, alpha, beta)
        for uplo, k in (("U", 0), ("L", -1), ("U", -64)):
            what = f"{dtype} {op} {uplo} {k} {c_case.shape()}"
            a, c = ref.fresh()[0]
            da, dc = dev(a), dev(c)
            st0 = costa.get_stats()
            costa.transform_tri(a_case.make_layout(0, da.data_ptr(), 1, dtype),
                                c_case.make_layout(0, dc.data_ptr(), 1, dtype), comm, op, uplo, k,
                                alpha, beta)
            st = costa.get_stats()
            if dc.cpu().numpy().tobytes() != ref.expected(uplo, k)[0].tobytes():
                fail(f"{what}: result differs from the masked oracle")
            if st["pack_launches"] == st0["pack_launches"] or st["unpack_launches"] == st0["unpack_launches"]:
                fail(f"{what}: no pack or no unpack launch")
            if st["tri_items"] == st0["tri_items"]:
                fail(f"{what}: no edge sub-tile ran")
            n += 1
    # in-place fill of the strict lower triangle through the exchange
    size = 300
    m0 = oracle.gen(oracle.DOUBLE, 0x31, 0, size * size)
    dm = dev(m0)
    costa.transform_tri(BC(size, size, 32, 48).make_layout(0, dm.data_ptr(), 1, oracle.DOUBLE),
                        BC(size, size, 40, 24).make_layout(0, dm.data_ptr(), 1, oracle.DOUBLE), comm,
                        "T", "L", -1)
    before = m0.reshape(size, size, order="F")
    want = np.where(keep_mask(size, size, "L", -1), before.T, before)
    got = dm.cpu().numpy().view(np.float64).reshape(size, size, order="F")
    if np.asfortranarray(got).tobytes() != np.asfortranarray(want).tobytes():
        fail("in-place fill through the exchange")
    n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["tri_items"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
