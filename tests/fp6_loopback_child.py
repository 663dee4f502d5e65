"""Child process of test_gpu_fp6.py (run with COSTA_LOOPBACK=1 or 2): the three MXFP6 calls on the
204 x 156 geometry, 'T', go through PACK -> ncclSend/ncclRecv to self -> the UNPACK list on mx_kernel
(mode 2: half of the tiles, the rest through the concurrent LOCAL launch, both writing the same scale
tensor).  quantise packs fp32; dequantise and requantise pack the packed FP6 bytes with the 1-byte
copy kernel, the package counted in bytes (3 per 4 elements).  C and the scale bytes are compared bit
for bit with fp6_common.expected_transform_mx6.  Stops at the first failure ('FAIL ...', exit status
1); else prints 'OK <cases> <pack> <unpack> <local launches> <mx items>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
import fp6_common as f6  # noqa: E402
import mx_common as mc  # noqa: E402
from fp6_common import COLS, E2M3, E3M2, F, ROWS  # noqa: E402


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
    items0 = costa.mx_items()
    op, n = "T", 0
    a_case, c_case = f6.geometry("g204", op)
    for ta, tc, alpha, beta, a_axis, c_axis in ((F, E2M3, 0.75, 0.0, None, COLS), (E3M2, F, -0.5, 2.0, ROWS, None),
                                                (E2M3, E2M3, 1.03125, 0.0, COLS, ROWS)):
        what = f"{f6.NAMES[ta]}->{f6.NAMES[tc]} g204 {op} loopback {mode}"
        na, nc = a_case.buf_elems(0, 1), c_case.buf_elems(0, 1)
        a = mc.quant_data(0x71, na) if ta == F else f6.fp6_data(0x72, na)
        c = f6.fill(tc, 0x73, nc)
        am, an = a_case.shape()
        m, k = c_case.shape()
        sa = sc0 = None
        if ta != F:
            sa = mc.scale_bytes(0x74, (mc.n_blocks(am), an) if a_axis == ROWS else (mc.n_blocks(an), am))
        if tc != F:
            sc0 = np.zeros((mc.n_blocks(m), k) if c_axis == ROWS else (mc.n_blocks(k), m), np.uint8)
        exp, esc, _ = f6.expected_transform_mx6(ta, tc, op, alpha, beta, a_case, c_case, 1, [a], [c], sa=sa,
                                                a_axis=a_axis, c_axis=c_axis)
        try:
            f6.assert_data_finite(exp[0], tc, what)
        except AssertionError as e:
            fail(str(e))
        da, dc = dev(a), dev(c)
        dsa = dev(sa).view(sa.shape) if sa is not None else None
        dsc = dev(sc0).view(sc0.shape) if sc0 is not None else None
        i0, s0 = costa.mx_items(), costa.scaled_items()
        costa.transform_mx(f6.make_layout(costa, a_case, 0, da.data_ptr(), 1, ta),
                           f6.make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc), comm, op, alpha, beta,
                           a_scales=costa.mx_scales(dsa, a_axis, a_case.shape()) if dsa is not None else None,
                           c_scales=costa.mx_scales(dsc, c_axis, c_case.shape()) if dsc is not None else None)
        try:
            f6.assert_same(dc.cpu().numpy().view(np.float32 if tc == F else np.uint8), exp[0], tc, what)
        except AssertionError as e:
            fail(str(e))
        if dsc is not None and dsc.cpu().numpy().tobytes() != esc.tobytes():
            fail(what + ": scale bytes differ")
        if dsa is not None and dsa.cpu().numpy().tobytes() != sa.tobytes():
            fail(what + ": a_scales changed")
        if costa.mx_items() <= i0 or costa.scaled_items() != s0:
            fail(what + ": the MX kernel did not run the lists")
        n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"], costa.mx_items() - items0)


if __name__ == "__main__":
    main()
