"""Child process of test_gpu_mx_sr.py (run with COSTA_LOOPBACK=1 or 2): MX transforms with stochastic
rounding, 'T', go through PACK -> ncclSend/ncclRecv to self -> the UNPACK list on the SR instances of
mx_kernel (mode 2: half of the tiles, the rest through the concurrent LOCAL launch, both writing the
same scale tensor).  quantise fp32 -> e4m3 packs fp32, requantise e2m1 -> e2m1 and e2m3 -> e2m3 pack the
packed bytes.  C is compared bit for bit with mx_sr_common.expected_transform_mx_sr and the scale bytes
with the model's, which are those of the call without a seed.  Stops at the first failure ('FAIL ...',
exit status 1); else prints 'OK <cases> <pack> <unpack> <local launches>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
import fp4_common as f4  # noqa: E402
import fp6_common as f6  # noqa: E402
import mx_common as mc  # noqa: E402
import mx_sr_common as sr  # noqa: E402
from mx_sr_common import COLS, E2M3, E4M3, F, FP4, ROWS  # noqa: E402

CASES = ((F, E4M3, mc.geometry, "g203", 0.75, None, COLS, 0x5EED00000001),
         (FP4, FP4, f4.geometry, "g202", 0.625, COLS, ROWS, 0x5EED00000002),
         (E2M3, E2M3, f6.geometry, "g204", 0.625, ROWS, COLS, (1 << 63) + 3))


def dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def fail(msg):
    print("FAIL", msg)
    sys.exit(1)


def model(case):
    """the model half of a case (no GPU): inputs, expected outputs and the conditions of test_gpu_mx_sr.py"""
    ta, tc, geometry, geom, alpha, a_axis, c_axis, seed = case
    a_case, c_case = geometry(geom, "T")
    what = f"{sr.NAMES[ta]}->{sr.NAMES[tc]} {geom} T seed {seed:#x}"
    a = sr.source_data(ta, 0x71, a_case.buf_elems(0, 1))
    c = sr.family(tc)[3](tc, 0x73, c_case.buf_elems(0, 1))
    am, an = a_case.shape()
    sa = None
    if ta != F:
        sa = mc.scale_bytes(0x74, (mc.n_blocks(am), an) if a_axis == ROWS else (mc.n_blocks(an), am))
    r = sr.expected_transform_mx_sr(seed, ta, tc, "T", alpha, 0.0, a_case, c_case, 1, [a], [c], sa=sa, a_axis=a_axis,
                                    c_axis=c_axis)
    sr.assert_finite(r.exp[0], tc, what)
    r.shares.check(what)
    r.__dict__.update(a_case=a_case, c_case=c_case, a=a, c=c, sa=sa, what=what)
    return r


def main():
    mode = os.environ.get("COSTA_LOOPBACK")
    assert mode in ("1", "2")
    comm = costa.Comm.self(0)
    costa.get_stats(reset=True)
    n = 0
    for case in CASES:
        ta, tc, _, _, alpha, a_axis, c_axis, seed = case
        try:
            r = model(case)
        except AssertionError as e:
            fail(str(e))
        what = r.what + f" loopback {mode}"
        lay = sr.family(tc)[2]
        m, k = r.c_case.shape()
        sc0 = np.zeros((mc.n_blocks(m), k) if c_axis == ROWS else (mc.n_blocks(k), m), np.uint8)
        da, dc = dev(r.a), dev(r.c)
        dsa = dev(r.sa).view(r.sa.shape) if r.sa is not None else None
        dsc = dev(sc0).view(sc0.shape)
        i0, s0 = costa.mx_items(), costa.scaled_items()
        costa.transform_mx(lay(costa, r.a_case, 0, da.data_ptr(), 1, ta), lay(costa, r.c_case, 0, dc.data_ptr(), 1, tc),
                           comm, "T", alpha, 0.0,
                           a_scales=costa.mx_scales(dsa, a_axis, r.a_case.shape()) if dsa is not None else None,
                           c_scales=costa.mx_scales(dsc, c_axis, r.c_case.shape()), stochastic_seed=seed)
        try:
            sr.family(tc)[4](dc.cpu().numpy().view(np.uint8), r.exp[0], tc, what)
        except AssertionError as e:
            fail(str(e))
        if dsc.cpu().numpy().tobytes() != r.sc.tobytes():
            fail(what + ": scale bytes differ")
        if dsa is not None and dsa.cpu().numpy().tobytes() != r.sa.tobytes():
            fail(what + ": a_scales changed")
        if costa.mx_items() <= i0 or costa.scaled_items() != s0:
            fail(what + ": the MX kernel did not run the lists")
        n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"])


if __name__ == "__main__":
    main()
