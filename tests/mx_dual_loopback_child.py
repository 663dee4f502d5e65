"""Child process of test_gpu_mx_dual.py (run with COSTA_LOOPBACK=1 or 2): dual-output MX quantise of e4m3
(203 x 157) and e2m1 (202 x 158), 'T', through PACK -> ncclSend/ncclRecv to self -> the UNPACK list on
mx_dual_kernel (mode 2: half of the tiles, the rest through the concurrent LOCAL launch, both writing the
same two scale tensors).  The fp32 package is packed once.  C, Ct and both scale tensors are compared bit
for bit with the models of mx_dual_common.py.  Stops at the first failure ('FAIL ...', exit status 1); else
prints 'OK <cases> <pack> <unpack> <local launches>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
import mx_common as mc  # noqa: E402
import mx_dual_common as dc  # noqa: E402
import mx_sr_common as sr  # noqa: E402
from mx_dual_common import E4M3, F, FP4, NAMES  # noqa: E402
from mx_sr_common import COLS, ROWS  # noqa: E402


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
    op, n = "T", 0
    for tq, geom, c_axis, ct_axis in ((E4M3, "g203", COLS, ROWS), (FP4, "g202", ROWS, ROWS)):
        what = f"dual f32->{NAMES[tq]} {geom} {op} loopback {mode}"
        a_case, c_case = dc.geometry(tq, geom, op)
        ct_case = dc.twin(c_case, "C")
        fill, lay, same = sr.family(tq)[3], sr.family(tq)[2], sr.family(tq)[4]
        a = mc.quant_data(0x71, a_case.buf_elems(0, 1))
        c, ct = fill(tq, 0x73, c_case.buf_elems(0, 1)), fill(tq, 0x75, ct_case.buf_elems(0, 1))
        m, k = c_case.shape()
        (e1, s1, _), (e2, s2, _) = dc.expected_transform(tq, op, 0.75, a_case, c_case, ct_case, 1, [a], [c], [ct], c_axis,
                                                         ct_axis, mc.FLOOR)
        dc.assert_finite(e1 + e2, tq, what)
        da, dcb, dct = dev(a), dev(c), dev(ct)
        dsc = dev(np.zeros(dc.sc_shape(m, k, c_axis), np.uint8)).view(dc.sc_shape(m, k, c_axis))
        dsct = dev(np.zeros(dc.sc_shape(k, m, ct_axis), np.uint8)).view(dc.sc_shape(k, m, ct_axis))
        i0, x0 = costa.mx_dual_items(), costa.mx_items()
        p0 = costa.get_stats()["pack_bytes"]
        costa.transform_mx_dual(lay(costa, a_case, 0, da.data_ptr(), 1, F), lay(costa, c_case, 0, dcb.data_ptr(), 1, tq),
                                lay(costa, ct_case, 0, dct.data_ptr(), 1, tq), comm, op, 0.75,
                                c_scales=costa.mx_scales(dsc, c_axis, c_case.shape()),
                                ct_scales=costa.mx_scales(dsct, ct_axis, ct_case.shape()))
        try:
            same(dcb.cpu().numpy().view(np.uint8), e1[0], tq, what + ": C")
            same(dct.cpu().numpy().view(np.uint8), e2[0], tq, what + ": Ct")
        except AssertionError as e:
            fail(str(e))
        if dsc.cpu().numpy().tobytes() != s1.tobytes() or dsct.cpu().numpy().tobytes() != s2.tobytes():
            fail(what + ": scale bytes differ")
        if da.cpu().numpy().tobytes() != a.tobytes():
            fail(what + ": A changed")
        if costa.mx_dual_items() <= i0 or costa.mx_items() != x0:
            fail(what + ": the dual kernel did not run the lists")
        # the fp32 package is packed once: at most A's elements, read and written as fp32
        if costa.get_stats()["pack_bytes"] - p0 > 8 * m * k:
            fail(what + ": more than one fp32 package was packed")
        n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"])


if __name__ == "__main__":
    main()
