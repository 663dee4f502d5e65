"""MXFP4 legs of transform_mx beside the MXFP8 (e4m3) legs of the same geometry, on one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), alpha, beta = 1, 0, rounding floor.  Legs:
    quantise 'N', 'T'        fp32 -> Q, blocks of C along rows
    requantise 'T' r->c      Q (blocks along A's rows) -> Q (blocks along C's columns)
    requantise 'T' c->c      Q (blocks along A's columns) -> Q (blocks along C's columns): every block
                             is cut anew; not expressible as a byte (let alone nibble) transposition
    dequantise 'N', 'T'      Q (blocks along rows) -> fp32
with Q = packed e2m1 (two codes per byte; the leg under test) and Q = e4m3 (the reference: the existing
transform_mx call of the same layouts, axes and op).  The reference of every ratio is the e4m3 call,
not the code under test.  An FP4 leg moves fewer bytes than its e4m3 counterpart (half on every Q
side), so fp4 / e4m3 below 1 is what the bytes alone would give.

All legs run in one process, stream-ordered, timed by device events around `--reps` calls after
`--warmup` calls of each; the legs alternate over `--rounds` rounds and the medians of the per-call
round means are reported with their min .. max.  Before the timing every FP4 leg is compared, bit for
bit over the whole matrix and the whole scale tensor, with the format's arithmetic written in torch on
the GPU (costa_hip.h, "MXFP4": seven midpoint comparisons for cvt4, a table for w4).

    python tools/bench_fp4.py [--reps 10] [--rounds 5] [--warmup 3] [--small] [--out FILE]
Prints one JSON line per leg and a markdown table; --small runs 2048^2 (a dry run of the script).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import costa_amd as costa  # noqa: E402

F, Q8, Q4 = "f32", "e4m3", "e2m1"
CODE = {F: costa.FLOAT, Q8: costa.FP8_E4M3, Q4: costa.FP4_E2M1}
BLOCK = 256
ROWS, COLS = costa.MX_ROWS, costa.MX_COLS
# (name, A is Q, C is Q, op, a_axis, c_axis)
LEGS = [
    ("quantise", False, True, "N", None, ROWS),
    ("quantise", False, True, "T", None, ROWS),
    ("requantise r->c", True, True, "T", ROWS, COLS),
    ("requantise c->c", True, True, "T", COLS, COLS),
    ("dequantise", True, False, "N", ROWS, None),
    ("dequantise", True, False, "T", ROWS, None),
]
MIDS = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]      # ties: 0.25, 1.25, 2.5, 5 down; 0.75, 1.75, 3.5 up
UP = [False, True, False, True, False, True, False]


def nbytes(n, kind):
    return n * n * 4 if kind == F else n * n if kind == Q8 else n * n // 2


def layout(n, t, kind):
    return costa.block_cyclic_layout(n, n, BLOCK, BLOCK, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     CODE[kind])


# Column-major storage: view(n, n)[j, i] is element (i, j).  A scale tensor is kept in the shape torch's
# reduction gives: blocks along rows -> [line j, block b] (line-major: block_stride 1), blocks along
# columns -> [block b, line i] (block-major).
def scale_tensor(n, axis, fill=None):
    shape = (n, n // 32) if axis == ROWS else (n // 32, n)
    t = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    if fill is not None:
        t.copy_(fill(shape))
    return t


def descriptor(t, axis):
    return costa.mx_scales(t.T if axis == ROWS else t, axis)


def blocks(v, n, axis):
    return (v.view(n, n // 32, 32), 2) if axis == ROWS else (v.view(n // 32, 32, n), 1)


def expand(sc, axis):
    p = (sc.to(torch.int32) << 23).view(torch.float32)
    return p.unsqueeze(2) if axis == ROWS else p.unsqueeze(1)


def w4(packed, n):
    """packed e2m1 bytes (column-major, rows share bytes) -> fp32 view(n, n)"""
    lut = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float32,
                       device="cuda")
    b = packed.view(n, n // 2).to(torch.int64)
    return lut[torch.stack((b & 15, b >> 4), dim=2).view(n, n)]


def cvt4_packed(t, n):
    """fp32 view(n, n) with |t| <= 6 -> packed bytes"""
    a = t.abs()
    m = torch.zeros_like(t, dtype=torch.uint8)
    for mid, up in zip(MIDS, UP):
        m += (a >= mid) if up else (a > mid)
    m |= (t.view(torch.int32) >> 28 & 8).to(torch.uint8)
    m = m.view(n, n // 2, 2)
    return (m[:, :, 0] | m[:, :, 1] << 4).reshape(-1)


def model(n, op, src, a_q, c_q, SA, a_axis, c_axis, sc_out):
    """the expected destination bytes of an FP4 leg (and sc_out filled), in torch on the GPU"""
    x = w4(src, n) if a_q else src.view(n, n)
    if a_q:
        b, _ = blocks(x.contiguous(), n, a_axis)
        x = (b * expand(SA, a_axis)).view(n, n)
    if op == "T":
        x = x.T.contiguous()
    if not c_q:
        return x.reshape(-1).view(torch.uint8)
    b, d = blocks(x.contiguous(), n, c_axis)
    e = b.abs().amax(dim=d).view(torch.int32) >> 23
    E = (e - 2).clamp_(0, 254)
    sc_out.copy_(E.to(torch.uint8))
    inv = ((254 - E) << 23).view(torch.float32).unsqueeze(d)
    return cvt4_packed((b * inv).clamp_(-6.0, 6.0).view(n, n), n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp4.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    n = 2048 if args.small else 16384
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    # uniform +-1 times 2^k, k per run of 32 stored elements: blocks of different exponents
    base = torch.rand(n * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1
    k = torch.randint(-6, 7, (n * n // 32,), device="cuda", generator=gen).repeat_interleave(32)
    base = base * torch.exp2(k.to(torch.float32))
    del k
    src = {F: base, Q8: base.to(torch.float8_e4m3fn).view(torch.uint8),
           Q4: torch.randint(0, 256, (n * n // 2,), dtype=torch.uint8, device="cuda", generator=gen)}
    dst = {kind: torch.zeros(nbytes(n, kind), dtype=torch.uint8, device="cuda") for kind in (F, Q8, Q4)}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    legs = []
    with torch.cuda.stream(s):
        for name, a_q, c_q, op, a_axis, c_axis in LEGS:
            rnd = lambda shape: torch.randint(120, 134, shape, dtype=torch.uint8, device="cuda", generator=gen)  # noqa: E731
            SA = scale_tensor(n, a_axis, rnd) if a_axis is not None else None
            for q in (Q4, Q8):
                ta, tc = (q if a_q else F), (q if c_q else F)
                A, C = src[ta], dst[tc]
                LA, LC = layout(n, A, ta), layout(n, C, tc)
                SC = scale_tensor(n, c_axis) if c_axis is not None else None
                da = descriptor(SA, a_axis) if SA is not None else None
                dc = descriptor(SC, c_axis) if SC is not None else None

                def call(LA=LA, LC=LC, op=op, da=da, dc=dc):
                    costa.transform_mx(LA, LC, comm, op, 1.0, 0.0, a_scales=da, c_scales=dc, stream=s)

                same = None
                if q == Q4:  # whole-matrix check of the FP4 leg
                    SC2 = scale_tensor(n, c_axis) if c_axis is not None else None
                    C.zero_()
                    call()
                    s.synchronize()
                    want = model(n, op, A, a_q, c_q, SA, a_axis, c_axis, SC2)
                    same = bool(torch.equal(want, C))
                    if SC is not None:
                        same = same and bool(torch.equal(SC, SC2))
                    del want
                legs.append({"leg": name, "op": op, "variant": q, "call": call, "check_passed": same,
                             "bytes": nbytes(n, ta) + nbytes(n, tc), "ms": []})
        for leg in legs:
            for _ in range(args.warmup):
                leg["call"]()
        s.synchronize()
        for _ in range(args.rounds):
            for leg in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(args.reps):
                    leg["call"]()
                e1.record(s)
                e1.synchronize()
                leg["ms"].append(e0.elapsed_time(e1) / args.reps)
    rows = []
    for leg in legs:
        ms = statistics.median(leg["ms"])
        rows.append({"leg": leg["leg"], "op": leg["op"], "variant": leg["variant"], "n": n, "block": BLOCK,
                     "check_passed": leg["check_passed"], "ms": round(ms, 4),
                     "ms_min_max": [round(min(leg["ms"]), 4), round(max(leg["ms"]), 4)],
                     "alg_bytes": leg["bytes"], "alg_gbs": round(leg["bytes"] / (ms * 1e-3) / 1e9, 1),
                     "reps": args.reps, "rounds": args.rounds})
    for r in rows:
        print(json.dumps(r), flush=True)
    lines = [f"| {n}^2, {BLOCK}^2 blocks | op | fp4 ms (min .. max) | GB/s | e4m3 ms (min .. max) | GB/s | "
             "fp4 / e4m3 | bytes fp4 / e4m3 | check |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, _, _, op, _, _ in LEGS:
        g = {r["variant"]: r for r in rows if r["leg"] == name and r["op"] == op}
        a, b = g[Q4], g[Q8]
        lines.append(f"| {name} | {op} | {a['ms']} ({a['ms_min_max'][0]} .. {a['ms_min_max'][1]}) | {a['alg_gbs']} "
                     f"| {b['ms']} ({b['ms_min_max'][0]} .. {b['ms_min_max'][1]}) | {b['alg_gbs']} "
                     f"| {a['ms'] / b['ms']:.3f} | {a['alg_bytes'] / b['alg_bytes']:.3f} | {a['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
