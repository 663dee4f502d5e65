"""Child process of test_gpu_bs.py (run with COSTA_LOOPBACK=1 or 2): block-scaled FP8 transforms of the
three call kinds on the 330 x 270 geometry with blocks on multiples of 128, 'T', go through PACK ->
ncclSend/ncclRecv to self -> the UNPACK list on block_kernel (mode 2: half of the tiles, the rest through
the concurrent LOCAL launch, both writing the same scale tensor).  quantise packs fp32, dequantise and
requantise pack FP8 bytes.  C and the scale floats are compared bit for bit with
bs_common.expected_transform_bs.  Stops at the first failure ('FAIL ...', exit status 1); else prints
'OK <cases> <pack> <unpack> <local launches>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
import bs_common as bc  # noqa: E402
from bs_common import E4M3, E5M2, F  # noqa: E402


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
    a_case, c_case = bc.geometry("bc128", op)
    for ta, tc, alpha, beta, a_block, c_block, rnd in ((F, E4M3, 0.75, 0.0, None, (128, 128), "exact"),
                                                       (E5M2, F, -0.5, 2.0, (1, 128), None, "exact"),
                                                       (E4M3, E4M3, 1.0, 0.0, (1, 128), (1, 128), "pow2")):
        what = f"{bc.NAMES[ta]}->{bc.NAMES[tc]} bc128 {op} loopback {mode}"
        na, nc = a_case.buf_elems(0, 1), c_case.buf_elems(0, 1)
        a = bc.quant_data(0x71, na) if ta == F else bc.cvt(bc.quant_data(0x72, na), ta)
        c = bc.fc.gen(tc, 0x73, nc)
        sa = sc0 = None
        if ta != F:
            sa = bc.scale_floats(0x74, bc.n_blocks(a_case.shape(), a_block))
        if tc != F:
            sc0 = np.zeros(bc.n_blocks(c_case.shape(), c_block), np.float32)
        exp, esc, _ = bc.expected_transform_bs(ta, tc, op, alpha, beta, a_case, c_case, 1, [a], [c], sa=sa,
                                               a_block=a_block, c_block=c_block,
                                               rounding=bc.POW2 if rnd == "pow2" else bc.EXACT)
        da, dc = dev(a), dev(c)
        dsa = torch.from_numpy(sa.copy()).cuda() if sa is not None else None
        dsc = torch.from_numpy(sc0.copy()).cuda() if sc0 is not None else None
        i0, s0, m0 = costa.block_items(), costa.scaled_items(), costa.mx_items()
        costa.transform_block_scaled(
            bc.make_layout(costa, a_case, 0, da.data_ptr(), 1, ta), bc.make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc),
            comm, op, alpha, beta,
            a_scales=costa.block_scales(dsa, a_block, a_case.shape()) if dsa is not None else None,
            c_scales=costa.block_scales(dsc, c_block, c_case.shape()) if dsc is not None else None, rounding=rnd)
        try:
            bc.assert_bits(dc.cpu().numpy().view(np.float32 if tc == F else np.uint8), exp[0], tc, what)
            if dsc is not None:
                bc.assert_float_bits(dsc.cpu().numpy(), esc, what + ": c_scales")
        except AssertionError as e:
            fail(str(e))
        if dsa is not None and dsa.cpu().numpy().tobytes() != sa.tobytes():
            fail(what + ": a_scales changed")
        if costa.block_items() <= i0 or costa.scaled_items() != s0 or costa.mx_items() != m0:
            fail(what + ": the block-scaled kernel did not run the lists")
        n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"])


if __name__ == "__main__":
    main()
