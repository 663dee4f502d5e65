"""The dual-output MX quantise beside the two separate transform_mx calls it replaces, on one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), fp32 source, alpha = 1, rounding floor, column-major A, C
and Ct, both scale tensors with their blocks along the columns of their own matrix (the reduction
dimensions of the forward and the backward GEMM).  Per type (e4m3, packed e2m1, packed e2m3), plain and
with a stochastic seed, three legs:
    dual   transform_mx_dual(A, C, Ct)              the code under test: A is read once
    N      transform_mx(A, C, 'N')                  the reference, unchanged code
    T      transform_mx(A, Ct, 'T')                 likewise; N + T is what a caller runs today
Before the timing the dual leg's C, Ct and both scale tensors are compared, byte for byte over the whole
matrices, with the N and the T leg's (fresh buffers).  All legs run in one process, stream-ordered, timed
by device events around `--reps` calls after `--warmup` calls of each; the N and the T leg follow the dual
leg inside every one of `--rounds` rounds.  Reported per leg: the median of the per-call round means with
its min .. max and the algorithmic GB/s; per type: dual / (N + T) as the ratio of medians with its
smallest and largest value over the rounds, and the spread (max - min over the rounds) of N + T, which
the gain has to exceed to be told from noise.

    python tools/bench_mx_dual.py [--reps 10] [--rounds 5] [--warmup 3] [--small] [--out FILE]
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

F, Q8, Q4, Q6 = "f32", "e4m3", "e2m1", "e2m3"
CODE = {F: costa.FLOAT, Q8: costa.FP8_E4M3, Q4: costa.FP4_E2M1, Q6: costa.FP6_E2M3}
BLOCK = 256
COLS = costa.MX_COLS
SEED = 0x0123456789ABCDEF


def nbytes(n, kind):
    return n * n * {F: 16, Q8: 4, Q4: 2, Q6: 3}[kind] // 4


def layout(n, t, kind):
    return costa.block_cyclic_layout(n, n, BLOCK, BLOCK, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     CODE[kind])


def scale_tensor(n):
    """blocks along columns: [block, line], block-major"""
    return torch.zeros((n // 32, n), dtype=torch.uint8, device="cuda")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mx_dual.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    n = 2048 if args.small else 16384
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    # (the data of bench_mx_sr.py) uniform +-1 times 2^k, k per run of 32 stored elements
    base = torch.rand(n * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1
    k = torch.randint(-6, 7, (n * n // 32,), device="cuda", generator=gen).repeat_interleave(32)
    base = base * torch.exp2(k.to(torch.float32))
    del k
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    groups = []
    with torch.cuda.stream(s):
        LA = layout(n, base, F)
        for q in (Q8, Q4, Q6):
            buf = [torch.zeros(nbytes(n, q), dtype=torch.uint8, device="cuda") for _ in range(4)]  # C, Ct, C', Ct'
            lay = [layout(n, b, q) for b in buf]
            sc = [scale_tensor(n) for _ in range(4)]
            desc = [costa.mx_scales(t, COLS) for t in sc]
            for variant, seed in (("plain", None), ("sr", SEED)):

                def dual(lay=lay, desc=desc, seed=seed):
                    costa.transform_mx_dual(LA, lay[0], lay[1], comm, "N", 1.0, c_scales=desc[0], ct_scales=desc[1],
                                            stochastic_seed=seed, stream=s)

                def leg_n(lay=lay, desc=desc, seed=seed):
                    costa.transform_mx(LA, lay[2], comm, "N", 1.0, 0.0, c_scales=desc[2], stochastic_seed=seed, stream=s)

                def leg_t(lay=lay, desc=desc, seed=seed):
                    costa.transform_mx(LA, lay[3], comm, "T", 1.0, 0.0, c_scales=desc[3], stochastic_seed=seed, stream=s)

                for t in buf + sc:
                    t.zero_()
                dual()
                leg_n()
                leg_t()
                s.synchronize()
                same = (bool(torch.equal(buf[0], buf[2])) and bool(torch.equal(buf[1], buf[3])) and
                        bool(torch.equal(sc[0], sc[2])) and bool(torch.equal(sc[1], sc[3])) and
                        bool(buf[0].any()) and bool(buf[1].any()) and bool(sc[0].any()) and bool(sc[1].any()))
                one = nbytes(n, F) + nbytes(n, q)
                groups.append({"type": q, "variant": variant, "check_passed": same,
                               "legs": [{"leg": "dual", "call": dual, "bytes": nbytes(n, F) + 2 * nbytes(n, q), "ms": []},
                                        {"leg": "N", "call": leg_n, "bytes": one, "ms": []},
                                        {"leg": "T", "call": leg_t, "bytes": one, "ms": []}]})
        for g in groups:
            for leg in g["legs"]:
                for _ in range(args.warmup):
                    leg["call"]()
        s.synchronize()
        for _ in range(args.rounds):
            for g in groups:
                for leg in g["legs"]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(args.reps):
                        leg["call"]()
                    e1.record(s)
                    e1.synchronize()
                    leg["ms"].append(e0.elapsed_time(e1) / args.reps)
    rows = []
    lines = [f"| {n}^2, {BLOCK}^2 blocks | variant | dual ms (min .. max) | GB/s | N ms (min .. max) | GB/s | "
             "T ms (min .. max) | GB/s | N + T ms (min .. max) | dual / (N + T) (min .. max over rounds) | "
             "gain ms | spread of N + T ms | check |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for g in groups:
        cells = []
        for leg in g["legs"]:
            ms = statistics.median(leg["ms"])
            r = {"type": g["type"], "variant": g["variant"], "leg": leg["leg"], "n": n, "block": BLOCK,
                 "check_passed": g["check_passed"], "ms": round(ms, 4),
                 "ms_min_max": [round(min(leg["ms"]), 4), round(max(leg["ms"]), 4)],
                 "ms_rounds": [round(x, 4) for x in leg["ms"]], "alg_bytes": leg["bytes"],
                 "alg_gbs": round(leg["bytes"] / (ms * 1e-3) / 1e9, 1), "reps": args.reps, "rounds": args.rounds}
            rows.append(r)
            cells.append(f"{r['ms']} ({r['ms_min_max'][0]} .. {r['ms_min_max'][1]}) | {r['alg_gbs']}")
        d, a, b = (leg["ms"] for leg in g["legs"])
        sums = [x + y for x, y in zip(a, b)]
        ratios = [x / y for x, y in zip(d, sums)]
        med_sum = statistics.median(a) + statistics.median(b)
        gain, spread = med_sum - statistics.median(d), max(sums) - min(sums)
        rows[-3].update(dual_over_sum=round(statistics.median(d) / med_sum, 3),
                        dual_over_sum_min_max=[round(min(ratios), 3), round(max(ratios), 3)], gain_ms=round(gain, 4),
                        sum_spread_ms=round(spread, 4), sum_min_max=[round(min(sums), 4), round(max(sums), 4)])
        lines.append(f"| {g['type']} | {g['variant']} | {' | '.join(cells)} | {med_sum:.4f} ({min(sums):.4f} .. "
                     f"{max(sums):.4f}) | {statistics.median(d) / med_sum:.3f} ({min(ratios):.3f} .. {max(ratios):.3f}) | "
                     f"{gain:.4f} | {spread:.4f} | {g['check_passed']} |")
    for r in rows:
        print(json.dumps(r), flush=True)
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
