"""MX block-scaled transforms against the ordinary transform of the same pair and geometry, and
against the multi-pass alternative (the ordinary transform into an fp32 temporary, then torch passes
for the block abs-max, the scale, the clamp and the conversion), on one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), e4m3, alpha, beta = 1, 0, rounding floor.  Legs:
    quantise 'N', 'T'        fp32 -> e4m3, blocks of C along rows
    requantise 'T' r->c      e4m3 (blocks along A's rows) -> e4m3 (blocks along C's columns): the same
                             element sets, the axis flipped with the matrix
    requantise 'T' c->c      e4m3 (blocks along A's columns) -> e4m3 (blocks along C's columns): every
                             block is cut anew; not expressible as a byte transposition
    dequantise 'N'           e4m3 (blocks along rows) -> fp32
Each leg is timed beside
    ordinary    costa.transform of the same pair and geometry (no scales): mx / ordinary is the price of
                the block reduction and the scale bytes
    multi-pass  costa.transform into fp32 (the op applied there), then torch: [multiply by the expanded
                input scales,] reshape to blocks, abs().amax(), exponent arithmetic on the bit
                patterns, multiply, clamp, .to(float8_e4m3fn); dequantise: the transform, then the
                multiplication by the expanded scales in place
All run in one process, stream-ordered, timed by device events around `--reps` calls after `--warmup`
calls of each; the legs alternate over `--rounds` rounds and the medians of the per-call round means
are reported with their spread.  Before the timing every MX leg is compared, bit for bit over the whole
matrix and the whole scale tensor, with torch's own arithmetic on the same data (the conversion to e4m3
on the CPU, the one the library is pinned to).

    python tools/bench_mx.py [--reps 10] [--rounds 5] [--warmup 3] [--small] [--out FILE]
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

Q = torch.float8_e4m3fn
F = torch.float32
BLOCK = 256
EMAX, FMAX = 8, 448.0
ROWS, COLS = costa.MX_ROWS, costa.MX_COLS
# (name, A dtype, C dtype, op, a_axis, c_axis)
LEGS = [
    ("quantise", F, Q, "N", None, ROWS),
    ("quantise", F, Q, "T", None, ROWS),
    ("requantise r->c", Q, Q, "T", ROWS, COLS),
    ("requantise c->c", Q, Q, "T", COLS, COLS),
    ("dequantise", Q, F, "N", ROWS, None),
]


def layout(n, t):
    return costa.block_cyclic_layout(n, n, BLOCK, BLOCK, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     costa.element_code(t.dtype))


def zeros(n, dt):
    return torch.zeros(n * n, dtype=torch.uint8, device="cuda").view(dt) if dt == Q \
        else torch.zeros(n * n, dtype=dt, device="cuda")


# Column-major storage: t.view(n, n)[j, i] is element (i, j).  A scale tensor is kept in the shape
# torch's reduction gives: blocks along rows -> [line j, block b] (line-major: block_stride 1), blocks
# along columns -> [block b, line i] (block-major).
def scale_tensor(n, axis, fill=None):
    shape = (n, n // 32) if axis == ROWS else (n // 32, n)
    t = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    if fill is not None:
        t.copy_(fill(shape))
    return t


def descriptor(t, axis):
    return costa.mx_scales(t.T if axis == ROWS else t, axis)


def blocks(v, n, axis):
    """the n x n view cut into blocks: the block's 32 elements along dim `d`"""
    return (v.view(n, n // 32, 32), 2) if axis == ROWS else (v.view(n // 32, 32, n), 1)


def expand(sc, n, axis):
    """pow2 of scale bytes (1 <= E <= 254 here) as fp32, one per block, broadcastable over blocks()"""
    p = (sc.to(torch.int32) << 23).view(torch.float32)
    return p.unsqueeze(2) if axis == ROWS else p.unsqueeze(1)


def quantise_passes(tmp, n, axis, sc_out, convert):
    """the torch passes of the multi-pass alternative on the fp32 matrix tmp -> e4m3 bits"""
    b, d = blocks(tmp.view(n, n), n, axis)
    amax = b.abs().amax(dim=d)
    e = amax.view(torch.int32) >> 23
    E = (e - EMAX).clamp_(0, 254)
    sc_out.copy_(E.to(torch.uint8))
    inv = ((254 - E) << 23).view(torch.float32).unsqueeze(d)
    return convert((b * inv).clamp_(-FMAX, FMAX))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mx.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    n = 2048 if args.small else 16384
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    # uniform +-1 times 2^k, k per run of 32 stored elements: blocks of different exponents
    base = torch.rand(n * n, dtype=F, device="cuda", generator=gen) * 2 - 1
    k = torch.randint(-6, 7, (n * n // 32,), device="cuda", generator=gen).repeat_interleave(32)
    base = base * torch.exp2(k.to(F))
    del k
    src = {F: base, Q: base.cpu().to(Q).cuda()}
    dst = {F: zeros(n, F), Q: zeros(n, Q)}
    tmp = zeros(n, F)
    LT = layout(n, tmp)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    legs = []
    with torch.cuda.stream(s):
        for name, ta, tc, op, a_axis, c_axis in LEGS:
            A, C = src[ta], dst[tc]
            LA, LC = layout(n, A), layout(n, C)
            rnd = lambda shape: torch.randint(120, 134, shape, dtype=torch.uint8, device="cuda", generator=gen)  # noqa: E731
            SA = scale_tensor(n, a_axis, rnd) if a_axis is not None else None
            SC = scale_tensor(n, c_axis) if c_axis is not None else None
            SC2 = scale_tensor(n, c_axis) if c_axis is not None else None
            da = descriptor(SA, a_axis) if SA is not None else None
            dc = descriptor(SC, c_axis) if SC is not None else None
            # SA in target coordinates: A's rows are C's columns for 'T'
            t_axis = a_axis if op == "N" or a_axis is None else (COLS if a_axis == ROWS else ROWS)

            def sa_target(SA=SA, op=op):
                return SA if op == "N" else SA.T

            def mx(LA=LA, LC=LC, op=op, da=da, dc=dc):
                costa.transform_mx(LA, LC, comm, op, 1.0, 0.0, a_scales=da, c_scales=dc, stream=s)

            def ordinary(LA=LA, LC=LC, op=op):
                costa.transform_async(LA, LC, comm, op, 1, 0, stream=s)

            def multi(convert=lambda x: x.to(Q), LA=LA, LC=LC, C=C, op=op, tc=tc, SA=SA, SC2=SC2, c_axis=c_axis,
                      t_axis=t_axis, sa_target=sa_target):
                out = tmp if tc == Q else C
                costa.transform_async(LA, LT if tc == Q else LC, comm, op, 1, 0, stream=s)
                if SA is not None:
                    b, _ = blocks(out.view(n, n), n, t_axis)
                    b.mul_(expand(sa_target().contiguous(), n, t_axis))
                if tc == Q:
                    q = quantise_passes(out, n, c_axis, SC2, convert)
                    C.view(n, n).view(torch.uint8).copy_(q.reshape(n, n).view(torch.uint8))

            # whole-matrix check of the MX leg: the multi-pass arithmetic with the CPU's conversion
            C.view(torch.uint8).zero_()
            multi(convert=lambda x: x.cpu().to(Q).cuda())
            s.synchronize()
            want = C.view(torch.uint8).clone()
            C.view(torch.uint8).zero_()
            mx()
            s.synchronize()
            same = bool(torch.equal(want, C.view(torch.uint8)))
            if SC is not None:
                same = same and bool(torch.equal(SC, SC2))
            del want
            for variant, call in (("mx", mx), ("ordinary", ordinary), ("multi-pass", multi)):
                legs.append({"leg": name, "op": op, "variant": variant, "call": call,
                             "check_passed": same if variant == "mx" else None,
                             "bytes": n * n * (A.element_size() + C.element_size()), "ms": []})
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
    lines = [f"| {n}^2, {BLOCK}^2 blocks | op | mx ms (min .. max) | GB/s | ordinary ms | multi-pass ms | "
             "mx / ordinary | mx / multi-pass | check |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, _, _, op, _, _ in LEGS:
        g = {r["variant"]: r for r in rows if r["leg"] == name and r["op"] == op}
        mxr, od, mp = g["mx"], g["ordinary"], g["multi-pass"]
        lines.append(f"| {name} | {op} | {mxr['ms']} ({mxr['ms_min_max'][0]} .. {mxr['ms_min_max'][1]}) "
                     f"| {mxr['alg_gbs']} | {od['ms']} | {mp['ms']} | {mxr['ms'] / od['ms']:.3f} "
                     f"| {mxr['ms'] / mp['ms']:.3f} | {mxr['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
