"""Child process of test_gpu_fp8.py (run with COSTA_LOOPBACK=1 or 2): FP8 transforms of the three
pair shapes -- e4m3 -> e4m3, fp32 -> e5m2, e4m3 -> fp32 -- on the 203 x 157 block-cyclic case 'T'
(alpha, beta) and on the custom-layout case cfg5 'N' go through PACK -> ncclSend/ncclRecv to self
-> UNPACK (mode 2: half of the tiles, the rest through the concurrent LOCAL launch).  The package
holds A's type: Q sources are byte-copied while packing (on the FP8 kernels), FLOAT sources are
packed unrounded by the same-type FLOAT kernels, and UNPACK converts.  Each result is compared byte
for byte with the CPU oracle run in FLOAT (fp8_common.expected_transform), hence with what the
LOCAL list gives, and the algorithmic byte counts of the pack and unpack lists with what the
package type gives.  Stops at the first failure ('FAIL ...', exit status 1); else prints
'OK <cases> <pack> <unpack> <local launches>'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import costa_amd as costa  # noqa: E402
from fp8_common import E4M3, E5M2, ESIZE, F, NAMES, expected_transform, gen, geometry, make_layout  # noqa: E402

SAME_TYPE_ITEMS = ("tile_items", "skew_items", "cblock_items", "tiny_items")


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
    for ta, tc in ((E4M3, E4M3), (F, E5M2), (E4M3, F)):
        for geom, op, alpha, beta in (("bc203", "T", -0.5, 2.0), ("cfg5", "N", 1, 0)):
            what = f"{NAMES[ta]}->{NAMES[tc]} {geom} {op}"
            a_case, c_case = geometry(geom, op)
            total = int(c_case.shape()[0]) * int(c_case.shape()[1])
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
            # the package holds A's type: pack moves E_A + E_A bytes per element, unpack E_A + E_C
            # (+ E_C when beta != 0)
            ea, ec = ESIZE[ta], ESIZE[tc]
            ep = ea
            pb = st["pack_bytes"] - st0["pack_bytes"]
            ub = st["unpack_bytes"] - st0["unpack_bytes"]
            if pb <= 0 or pb % (ea + ep):
                fail(f"{what}: pack_bytes {pb} is no multiple of {ea + ep}")
            moved = pb // (ea + ep)
            if mode == "1" and moved != total:
                fail(f"{what}: {moved} elements packed, {total} expected")
            if mode == "2" and not 0 < moved < total:
                fail(f"{what}: {moved} elements packed of {total}")
            if ub != moved * (ep + ec * (2 if beta else 1)):
                fail(f"{what}: unpack_bytes {ub} for {moved} elements")
            # LOCAL and UNPACK run on the FP8 family, and PACK too when A holds Q; a FLOAT source
            # is packed by the same-type kernels
            same = any(st[k] != st0[k] for k in SAME_TYPE_ITEMS)
            if ta == F and not same:
                fail(f"{what}: the FLOAT package was not packed by the same-type kernels")
            if ta != F and same:
                fail(f"{what}: a list ran on the same-type kernels")
            if st["convert_items"] == st0["convert_items"]:
                fail(f"{what}: no converting sub-tile ran")
            n += 1
    st = costa.get_stats()
    print("OK", n, st["pack_launches"], st["unpack_launches"], st["local_launches"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
