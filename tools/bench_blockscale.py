"""Block-scaled FP8 transforms (fp32 scales per 1 x 128 / 128 x 128 block) against the MX transform of
the same pair and geometry, and against the multi-pass alternative (the ordinary transform into an fp32
temporary, then torch passes for the block abs-max, the divisions, the clamp and the conversion), on
one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), e4m3, alpha, beta = 1, 0, rounding exact.  Legs:
    quantise 'N', 'T' 1x128      fp32 -> e4m3, one scale per 128 consecutive columns of a row of C
    quantise 'N' 128x128         fp32 -> e4m3, one scale per tile of C (weights)
    requantise 'T' 1x128->1x128  e4m3 in 1 x 128 groups of A -> groups along the OTHER dimension: 1 x 128
                                 groups of the transposed matrix; every block is cut anew
    dequantise 'N' 1x128         e4m3 -> fp32
Each leg is timed beside
    mx          costa.transform_mx of the same pair and geometry (E8M0 bytes per 32 elements along the
                same direction; 128 x 128: along rows)
    multi-pass  costa.transform into fp32 (the op applied there), then torch: [multiply by the expanded
                input scales,] reshape to blocks, abs().amax(), clamp_min(2^-40), the two divisions,
                multiply, clamp, .to(float8_e4m3fn); dequantise: the transform, then the multiplication
                by the expanded scales in place
All run in one process, stream-ordered, timed by device events around `--reps` calls after `--warmup`
calls of each; the legs alternate over `--rounds` rounds and the medians of the per-call round means
are reported with their spread.  Before the timing every fused leg is compared, bit for bit over the
whole matrix and the whole scale tensor, with torch's own arithmetic on the same data (the conversion
to e4m3 and the divisions of the block maxima on the CPU, the ones the library is pinned to).

    python tools/bench_blockscale.py [--reps 10] [--rounds 5] [--warmup 3] [--small] [--out FILE]
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
FMAX, EPS = 448.0, 2.0 ** -40
ROWS, COLS = costa.MX_ROWS, costa.MX_COLS
# (name, A dtype, C dtype, op, a_block, c_block, the MX axes of the counterpart)
LEGS = [
    ("quantise 1x128", F, Q, "N", None, (1, 128), (None, COLS)),
    ("quantise 1x128", F, Q, "T", None, (1, 128), (None, COLS)),
    ("quantise 128x128", F, Q, "N", None, (128, 128), (None, ROWS)),
    ("requantise 1x128->1x128", Q, Q, "T", (1, 128), (1, 128), (COLS, COLS)),
    ("dequantise 1x128", Q, F, "N", (1, 128), None, (COLS, None)),
]


def layout(n, t):
    return costa.block_cyclic_layout(n, n, BLOCK, BLOCK, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     costa.element_code(t.dtype))


def zeros(n, dt):
    return torch.zeros(n * n, dtype=torch.uint8, device="cuda").view(dt) if dt == Q \
        else torch.zeros(n * n, dtype=dt, device="cuda")


# Column-major storage: t.view(n, n)[j, i] is element (i, j).  A scale tensor is kept in the shape torch's
# reduction gives, [block column, block row]; the descriptor takes its transpose (a view).
def blocks(v, n, block):
    br, bc = block
    return v.view(n // bc, bc, n // br, br)


def scale_tensor(n, block, fill=None):
    t = torch.zeros((n // block[1], n // block[0]), dtype=F, device="cuda")
    if fill is not None:
        t.copy_(fill(t.shape))
    return t


def expand(sc):
    return sc.unsqueeze(1).unsqueeze(3)


def quantise_passes(tmp, n, block, sc_out, convert, on_cpu=False):
    """the torch passes of the multi-pass alternative on the fp32 matrix tmp -> e4m3 bits; on_cpu (the
    check): the two divisions of the small amax tensor are made on the CPU, where torch's fp32 division
    is correctly rounded whatever the GPU build's is"""
    b = blocks(tmp.view(n, n), n, block)
    amax = b.abs().amax(dim=(1, 3)).clamp_min_(EPS)
    if on_cpu:
        a = amax.cpu()
        fm = torch.full_like(a, FMAX)  # (tensor / tensor: `scalar / tensor` is reciprocal-then-multiply)
        S, R = (a / fm).cuda(), (fm / a).cuda()
    else:
        fm = torch.full_like(amax, FMAX)
        S, R = amax / fm, fm / amax
    sc_out.copy_(S)
    return convert((b * expand(R)).clamp_(-FMAX, FMAX))


def mx_scale_tensor(n, axis):
    return torch.zeros((n, n // 32) if axis == ROWS else (n // 32, n), dtype=torch.uint8, device="cuda")


def mx_descriptor(t, axis):
    return costa.mx_scales(t.T if axis == ROWS else t, axis)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_blockscale.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    n = 2048 if args.small else 16384
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    # uniform +-1 times 2^k, k per run of 32 stored elements: blocks of different maxima
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
        for name, ta, tc, op, a_block, c_block, (mx_a, mx_c) in LEGS:
            A, C = src[ta], dst[tc]
            LA, LC = layout(n, A), layout(n, C)
            rnd = lambda shape: torch.rand(shape, dtype=F, device="cuda", generator=gen) * 0.03 + 0.001  # noqa: E731
            SA = scale_tensor(n, a_block, rnd) if a_block else None
            SC = scale_tensor(n, c_block) if c_block else None
            SC2 = scale_tensor(n, c_block) if c_block else None
            da = costa.block_scales(SA.T, a_block, (n, n)) if a_block else None
            dc = costa.block_scales(SC.T, c_block, (n, n)) if c_block else None
            # SA in target coordinates: A's rows are C's columns for 'T'
            t_block = a_block if op == "N" or not a_block else (a_block[1], a_block[0])
            MA = mx_scale_tensor(n, mx_a).fill_(125) if mx_a is not None else None
            MC = mx_scale_tensor(n, mx_c) if mx_c is not None else None
            ma = mx_descriptor(MA, mx_a) if MA is not None else None
            mc = mx_descriptor(MC, mx_c) if MC is not None else None

            def fused(LA=LA, LC=LC, op=op, da=da, dc=dc):
                costa.transform_block_scaled(LA, LC, comm, op, 1.0, 0.0, a_scales=da, c_scales=dc, stream=s)

            def mx(LA=LA, LC=LC, op=op, ma=ma, mc=mc):
                costa.transform_mx(LA, LC, comm, op, 1.0, 0.0, a_scales=ma, c_scales=mc, stream=s)

            def multi(convert=lambda x: x.to(Q), on_cpu=False, LA=LA, LC=LC, C=C, op=op, tc=tc, SA=SA, SC2=SC2, c_block=c_block,
                      t_block=t_block):
                out = tmp if tc == Q else C
                costa.transform_async(LA, LT if tc == Q else LC, comm, op, 1, 0, stream=s)
                if SA is not None:
                    blocks(out.view(n, n), n, t_block).mul_(expand(SA if op == "N" else SA.T))
                if tc == Q:
                    q = quantise_passes(out, n, c_block, SC2, convert, on_cpu)
                    C.view(n, n).view(torch.uint8).copy_(q.reshape(n, n).view(torch.uint8))

            # whole-matrix check of the fused leg: the multi-pass arithmetic with the CPU's conversion
            C.view(torch.uint8).zero_()
            multi(convert=lambda x: x.cpu().to(Q).cuda(), on_cpu=True)
            s.synchronize()
            want = C.view(torch.uint8).clone()
            C.view(torch.uint8).zero_()
            fused()
            s.synchronize()
            n_data = int((want != C.view(torch.uint8)).sum())
            n_scale = int((SC.view(torch.int32) != SC2.view(torch.int32)).sum()) if SC is not None else 0
            same = n_data == 0 and n_scale == 0
            if not same:
                print(f"check {name} {op}: {n_data} data bytes and {n_scale} scale floats differ", flush=True)
            del want
            for variant, call in (("fused", fused), ("mx", mx), ("multi-pass", multi)):
                legs.append({"leg": name, "op": op, "variant": variant, "call": call,
                             "check_passed": same if variant == "fused" else None,
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
    lines = [f"| {n}^2, {BLOCK}^2 blocks | op | fused ms (min .. max) | GB/s | mx ms | multi-pass ms | "
             "fused / mx | fused / multi-pass | check |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, _, _, op, _, _, _ in LEGS:
        g = {r["variant"]: r for r in rows if r["leg"] == name and r["op"] == op}
        fu, mxr, mp = g["fused"], g["mx"], g["multi-pass"]
        lines.append(f"| {name} | {op} | {fu['ms']} ({fu['ms_min_max'][0]} .. {fu['ms_min_max'][1]}) "
                     f"| {fu['alg_gbs']} | {mxr['ms']} | {mp['ms']} | {fu['ms'] / mxr['ms']:.3f} "
                     f"| {fu['ms'] / mp['ms']:.3f} | {fu['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
