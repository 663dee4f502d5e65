"""Child process of test_gpu_half.py (run with COSTA_LOOPBACK=1 or 2): half-precision transforms
of the 203 x 157 block-cyclic case -- bf16 -> bf16, fp32 -> bf16, bf16 -> fp32 and fp16 -> fp16,
'N' and 'T' with alpha, beta -- go through PACK -> ncclSend/ncclRecv to self -> UNPACK (mode 2:
half of the tiles, the rest through the concurrent LOCAL launch).  The package holds the 2-byte
type for every pair: FLOAT sources are rounded while packing, FLOAT targets widened while
unpacking.  Each result is compared bit for bit with the CPU oracle run in FLOAT
(half_common.expected_transform), and the algorithmic byte counts of the pack and unpack lists with
what a 2-byte package gives.  Stops at the first failure ('FAIL ...', exit status 1); else prints
'OK <cases> <pack> <unpack> <local launches>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
from half_common import BF16, ESIZE, F, H16, NAMES, expected_transform, gen, geometry, make_layout  # noqa: E402

M, N = 203, 157


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
    for ta, tc in ((BF16, BF16), (F, BF16), (BF16, F), (H16, H16)):
        for op, alpha, beta in (("N", 1, 0), ("T", -0.5, 2.0)):
            what = f"{NAMES[ta]}->{NAMES[tc]} {op}"
            a_case, c_case = geometry("bc203", op)
            a = gen(ta, 0x71, a_case.buf_elems(0, 1))
            c = gen(tc, 0x72, c_case.buf_elems(0, 1))
            exp = expected_transform(ta, tc, op, alpha, beta, a_case, c_case, a, c)
            da, dc = dev(a), dev(c)
            st0 = costa.get_stats()
            costa.transform(make_layout(costa, a_case, 0, da.data_ptr(), 1, ta),
                            make_layout(costa, c_case, 0, dc.data_ptr(), 1, tc), comm, op, alpha, beta)
            st = costa.get_stats()
            if dc.cpu().numpy().tobytes() != exp.tobytes():
                fail(f"{what}: result differs from the oracle")
            if st["pack_launches"] == st0["pack_launches"] or st["unpack_launches"] == st0["unpack_launches"]:
                fail(f"{what}: no pack or no unpack launch")
            if mode == "1" and st["local_launches"] != st0["local_launches"]:
                fail(f"{what}: a local launch in mode 1")
            # the package holds H: pack moves E_A + 2 bytes per element, unpack 2 + E_C (+ E_C when
            # beta != 0)
            ea, ec, ep = ESIZE[ta], ESIZE[tc], 2
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
            # every list of a half-precision plan runs on the converting family
            for k in ("tile_items", "skew_items", "cblock_items", "tiny_items"):
                if st[k] != st0[k]:
                    fail(f"{what}: {k} moved: a list ran on the same-type kernels")
            if st["convert_items"] == st0["convert_items"]:
                fail(f"{what}: no converting sub-tile ran")
            n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
