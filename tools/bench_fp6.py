"""MXFP6 legs of transform_mx beside the MXFP8 (e4m3) and MXFP4 (e2m1) legs of the same geometry, on
one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), alpha, beta = 1, 0, rounding floor.  Legs:
    quantise 'N', 'T'        fp32 -> Q, blocks of C along rows
    requantise 'T' r->c      Q (blocks along A's rows) -> Q (blocks along C's columns)
    requantise 'T' c->c      Q (blocks along A's columns) -> Q (blocks along C's columns): every block
                             is cut anew, and every 6-bit code moves to another bit position
    dequantise 'N', 'T'      Q (blocks along rows) -> fp32
with Q = packed e2m3 (four codes per three bytes; the legs under test), Q = packed e3m2 for one leg per
kind (the codec should not matter), and Q = e4m3 and Q = packed e2m1: the references, the existing
transform_mx calls of the same layouts, axes and op, not the code under test.  An FP6 side moves 0.75
of the bytes of an e4m3 side and 1.5 times those of an e2m1 side; the byte ratios of whole calls stand
beside the time ratios.

All legs run in one process, stream-ordered, timed by device events around `--reps` calls after
`--warmup` calls of each; the legs alternate over `--rounds` rounds and the medians of the per-call
round means are reported with their min .. max.  Before the timing every FP6 leg is compared, bit for
bit over the whole matrix and the whole scale tensor, with the format's arithmetic written in torch on
the GPU (costa_hip.h, "MXFP6": a 64-entry table for w6, 31 midpoint comparisons for cvt6).

    python tools/bench_fp6.py [--reps 10] [--rounds 5] [--warmup 3] [--small] [--out FILE]
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

F, Q8, Q4, Q6A, Q6B = "f32", "e4m3", "e2m1", "e2m3", "e3m2"
CODE = {F: costa.FLOAT, Q8: costa.FP8_E4M3, Q4: costa.FP4_E2M1, Q6A: costa.FP6_E2M3, Q6B: costa.FP6_E3M2}
FP6 = {Q6A: dict(mb=3, bias=1, emax=2, fmax=7.5), Q6B: dict(mb=2, bias=3, emax=4, fmax=28.0)}
BLOCK = 256
ROWS, COLS = costa.MX_ROWS, costa.MX_COLS
# (name, A is Q, C is Q, op, a_axis, c_axis, also timed for e3m2)
LEGS = [
    ("quantise", False, True, "N", None, ROWS, True),
    ("quantise", False, True, "T", None, ROWS, False),
    ("requantise r->c", True, True, "T", ROWS, COLS, True),
    ("requantise c->c", True, True, "T", COLS, COLS, False),
    ("dequantise", True, False, "N", ROWS, None, True),
    ("dequantise", True, False, "T", ROWS, None, False),
]


def nbytes(n, kind):
    return n * n * 4 if kind == F else n * n if kind == Q8 else n * n // 2 if kind == Q4 else n * n * 3 // 4


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


def magnitudes(q):
    """the 32 magnitudes of an FP6 type, from the format's definition"""
    mb, bias = FP6[q]["mb"], FP6[q]["bias"]
    out = []
    for c in range(32):
        e, m = c >> mb, c & ((1 << mb) - 1)
        out.append(m / (1 << mb) * 2.0 ** (1 - bias) if e == 0 else (1 + m / (1 << mb)) * 2.0 ** (e - bias))
    return out


def w6(packed, n, q):
    """packed FP6 bytes (column-major, rows share 3-byte groups) -> fp32 view(n, n)"""
    mags = magnitudes(q)
    lut = torch.tensor(mags + [-x for x in mags], dtype=torch.float32, device="cuda")
    b = packed.view(n, n // 4, 3).to(torch.int32)
    w = b[:, :, 0] | b[:, :, 1] << 8 | b[:, :, 2] << 16
    codes = torch.stack([(w >> (6 * k)) & 63 for k in range(4)], dim=2).view(n, n)
    return lut[codes.to(torch.int64)]


def cvt6_packed(t, n, q):
    """fp32 view(n, n) with |t| <= fmax -> packed bytes: comparisons against the 31 midpoints, a tie to
    the code whose mantissa is even"""
    mags = magnitudes(q)
    a = t.abs()
    m = torch.zeros_like(t, dtype=torch.uint8)
    for k in range(31):
        mid = (mags[k] + mags[k + 1]) / 2
        m += (a >= mid) if k % 2 == 1 else (a > mid)       # odd k: the tie goes up to the even k + 1
    m |= (t.view(torch.int32) >> 26 & 32).to(torch.uint8)
    c = m.view(n, n // 4, 4).to(torch.int32)
    w = c[:, :, 0] | c[:, :, 1] << 6 | c[:, :, 2] << 12 | c[:, :, 3] << 18
    return torch.stack((w & 255, (w >> 8) & 255, w >> 16), dim=2).to(torch.uint8).reshape(-1)


def model(n, op, src, q, a_q, c_q, SA, a_axis, c_axis, sc_out):
    """the expected destination bytes of an FP6 leg (and sc_out filled), in torch on the GPU"""
    x = w6(src, n, q) if a_q else src.view(n, n)
    if a_q:
        b, _ = blocks(x.contiguous(), n, a_axis)
        x = (b * expand(SA, a_axis)).view(n, n)
    if op == "T":
        x = x.T.contiguous()
    if not c_q:
        return x.reshape(-1).view(torch.uint8)
    b, d = blocks(x.contiguous(), n, c_axis)
    e = b.abs().amax(dim=d).view(torch.int32) >> 23
    E = (e - FP6[q]["emax"]).clamp_(0, 254)
    sc_out.copy_(E.to(torch.uint8))
    inv = ((254 - E) << 23).view(torch.float32).unsqueeze(d)
    fm = FP6[q]["fmax"]
    return cvt6_packed((b * inv).clamp_(-fm, fm).view(n, n), n, q)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp6.py needs a GPU (there is no CPU path to time)")
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
    src[Q6A] = torch.randint(0, 256, (n * n * 3 // 4,), dtype=torch.uint8, device="cuda", generator=gen)
    src[Q6B] = src[Q6A]                                    # (every byte pattern is four valid codes)
    dst = {kind: torch.zeros(nbytes(n, kind), dtype=torch.uint8, device="cuda") for kind in (F, Q8, Q4, Q6A)}
    dst[Q6B] = dst[Q6A]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    legs = []
    with torch.cuda.stream(s):
        for name, a_q, c_q, op, a_axis, c_axis, both in LEGS:
            rnd = lambda shape: torch.randint(120, 134, shape, dtype=torch.uint8, device="cuda", generator=gen)  # noqa: E731
            SA = scale_tensor(n, a_axis, rnd) if a_axis is not None else None
            for q in (Q6A, Q6B, Q8, Q4):
                if q == Q6B and not both:
                    continue
                ta, tc = (q if a_q else F), (q if c_q else F)
                A, C = src[ta], dst[tc]
                LA, LC = layout(n, A, ta), layout(n, C, tc)
                SC = scale_tensor(n, c_axis) if c_axis is not None else None
                da = descriptor(SA, a_axis) if SA is not None else None
                dc = descriptor(SC, c_axis) if SC is not None else None

                def call(LA=LA, LC=LC, op=op, da=da, dc=dc):
                    costa.transform_mx(LA, LC, comm, op, 1.0, 0.0, a_scales=da, c_scales=dc, stream=s)

                same = None
                if q in FP6:  # whole-matrix check of the FP6 leg
                    SC2 = scale_tensor(n, c_axis) if c_axis is not None else None
                    C.zero_()
                    call()
                    s.synchronize()
                    want = model(n, op, A, q, a_q, c_q, SA, a_axis, c_axis, SC2)
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

    def cell(r):
        return f"{r['ms']} ({r['ms_min_max'][0]} .. {r['ms_min_max'][1]}) | {r['alg_gbs']}"
    lines = [f"| {n}^2, {BLOCK}^2 blocks | op | type | fp6 ms (min .. max) | GB/s | e4m3 ms (min .. max) | GB/s | "
             "e2m1 ms (min .. max) | GB/s | fp6 / e4m3 | bytes | fp6 / e2m1 | bytes | check |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, _, _, op, _, _, both in LEGS:
        g = {r["variant"]: r for r in rows if r["leg"] == name and r["op"] == op}
        for q in (Q6A, Q6B) if both else (Q6A,):
            a, b, c = g[q], g[Q8], g[Q4]
            lines.append(f"| {name} | {op} | {q} | {cell(a)} | {cell(b)} | {cell(c)} "
                         f"| {a['ms'] / b['ms']:.3f} | {a['alg_bytes'] / b['alg_bytes']:.3f} "
                         f"| {a['ms'] / c['ms']:.3f} | {a['alg_bytes'] / c['alg_bytes']:.3f} | {a['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
