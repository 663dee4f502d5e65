"""Child process of test_gpu_amax.py (run with COSTA_LOOPBACK=1 or 2): amax transforms of the pairs
fp32 -> fp32, fp32 -> bf16, e4m3 -> fp32, bf16 -> bf16 and fp64 -> fp64 on the 203 x 157
block-cyclic case 'T' with alpha and beta go through PACK -> ncclSend/ncclRecv to self -> the UNPACK
list on the amax instance of the scaled kernel (mode 2: half of the tiles, the rest through the
concurrent LOCAL launch, both updating the same vectors).  For fp32 -> bf16 the package holds bf16,
so the amax is that of the bf16-rounded values.  C is compared bit for bit with
scaled_common.expected_transform, the vectors with amax_common.expected_transform_amax.  Stops at the
first failure ('FAIL ...', exit status 1); else prints 'OK <cases> <pack> <unpack> <local launches>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
from amax_common import assert_moved, assert_vec, expected_transform_amax, matrix_data  # noqa: E402
from scaled_common import (BF16, D, E4M3, F, NAMES, NPT, assert_bits, assert_finite, ctype,  # noqa: E402
                           expected_transform, gen, geometry, make_layout, scales)


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
    op, alpha, beta = "T", -0.5, 2.0
    for ta, tc in ((F, F), (F, BF16), (E4M3, F), (BF16, BF16), (D, D)):
        what = f"{NAMES[ta]}->{NAMES[tc]} bc203 {op}"
        a_case, c_case = geometry("bc203", op)
        ct = ctype(ta, tc)
        m, k = c_case.shape()
        a = matrix_data(ta, 0x71, a_case)
        c = gen(tc, 0x72, c_case.buf_elems(0, 1))
        r, cs = scales(m, 0x73, ct), scales(k, 0x74, ct)
        exp = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c, r, cs)
        assert_finite(exp, tc, what)
        r0, c0 = np.zeros(m, ct), np.zeros(k, ct)
        er, ec = expected_transform_amax(ta, tc, op, a_case, c_case, a, r0, c0)
        assert_moved(er, r0, what)
        assert_moved(ec, c0, what)
        da, dc = dev(a), dev(c)
        dr, dcs = torch.from_numpy(r).cuda(), torch.from_numpy(cs).cuda()
        ra, ca = torch.from_numpy(r0).cuda(), torch.from_numpy(c0).cuda()
        st0, items0 = costa.get_stats(), costa.amax_items()
        costa.transform_amax(make_layout(costa, a_case, 0, da.data_ptr(), 1, ta),
                             make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc), comm, op, alpha, beta,
                             dr, dcs, ra, ca)
        st = costa.get_stats()
        try:
            assert_bits(dc.cpu().numpy().view(NPT[tc]), exp, tc, what)
            assert_vec(ra.cpu().numpy(), er, what + ": row_amax")
            assert_vec(ca.cpu().numpy(), ec, what + ": col_amax")
        except AssertionError as e:
            fail(str(e))
        if st["pack_launches"] == st0["pack_launches"] or st["unpack_launches"] == st0["unpack_launches"]:
            fail(f"{what}: no pack or no unpack launch")
        if mode == "1" and st["local_launches"] != st0["local_launches"]:
            fail(f"{what}: a local launch in mode 1")
        if costa.amax_items() == items0:
            fail(f"{what}: no amax sub-tile ran")
        n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
