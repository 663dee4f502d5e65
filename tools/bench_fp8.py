"""FP8 transforms against the FLOAT and the bf16 transform of the same geometry on one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), 'N' and 'T' with alpha, beta = 1, 0:
    e4m3 -> e4m3, fp32 -> e4m3, e4m3 -> fp32     (fp8_kernels.hip)
    fp32 -> fp32                                 (tile_kernels.hip: a yardstick)
    bf16 -> bf16                                 (half_kernels.hip: a yardstick)
All run in one process, stream-ordered as the headline benchmark does.  Each is timed by device
events on one stream around `--reps` calls, after `--warmup` calls of each (which also warm the plan
cache); the legs alternate over `--rounds` rounds and the medians of the per-call round means are
reported with their spread (min .. max), together with the algorithmic GB/s (n^2 elements read at
A's element size and written at C's) and the time per element relative to the FLOAT and to the
bf16 leg of the same op.  Before the timing every leg is compared, byte for byte over the whole
matrix, with torch's own cast (and transpose) of the same data.

    python tools/bench_fp8.py [--reps 20] [--rounds 7] [--warmup 5] [--small] [--out FILE]
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
# (name, A's torch dtype, C's torch dtype)
LEGS = [
    ("e4m3->e4m3", Q, Q),
    ("fp32->e4m3", torch.float32, Q),
    ("e4m3->fp32", Q, torch.float32),
    ("fp32->fp32", torch.float32, torch.float32),
    ("bf16->bf16", torch.bfloat16, torch.bfloat16),
]
BLOCK = 256


def layout(n, t):
    return costa.block_cyclic_layout(n, n, BLOCK, BLOCK, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     costa.element_code(t.dtype))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp8.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    n = 2048 if args.small else 16384
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    base = torch.rand(n * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1
    # the FP8 input is torch-CPU's conversion of the fp32 input (the conversion the library is
    # pinned to), so it is also the expected result of the fp32 -> e4m3 legs
    src = {Q: base.cpu().to(Q).cuda(), torch.bfloat16: base.to(torch.bfloat16), torch.float32: base}
    dst = {dt: torch.zeros(n * n, dtype=torch.uint8, device="cuda").view(dt) if dt == Q
           else torch.zeros(n * n, dtype=dt, device="cuda") for dt in (Q, torch.bfloat16, torch.float32)}
    del base
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    legs = []
    with torch.cuda.stream(s):
        for name, ta, tc in LEGS:
            A, C = src[ta], dst[tc]
            LA, LC = layout(n, A), layout(n, C)
            for op in ("N", "T"):
                def call(LA=LA, LC=LC, op=op):
                    costa.transform_async(LA, LC, comm, op, 1, 0, stream=s)
                # whole-matrix check against torch's cast (column-major storage: 'T' is the
                # transposed view); the result is verified before anything is timed
                C.view(torch.uint8).zero_()
                call()
                s.synchronize()
                # (same-type legs and fp32 -> e4m3: the bytes of the input of C's type; e4m3 -> fp32:
                # its exact widening)
                a = src[tc].view(torch.uint8).view(n, n, -1) if ta == tc or tc == Q else A.view(n, n, 1).to(tc)
                want = (a.transpose(0, 1) if op == "T" else a).contiguous()
                same = bool(torch.equal(want.view(-1).view(torch.uint8), C.view(torch.uint8)))
                del want
                legs.append({"leg": name, "op": op, "call": call, "check_passed": same,
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
        rows.append({"leg": leg["leg"], "op": leg["op"], "n": n, "block": BLOCK, "check_passed": leg["check_passed"],
                     "ms": round(ms, 4), "ms_min_max": [round(min(leg["ms"]), 4), round(max(leg["ms"]), 4)],
                     "alg_bytes": leg["bytes"], "alg_gbs": round(leg["bytes"] / (ms * 1e-3) / 1e9, 1),
                     "reps": args.reps, "rounds": args.rounds})
    for r in rows:  # time per element against both yardsticks of the same op, timed in the same rounds
        for key, name in (("time_over_float", "fp32->fp32"), ("time_over_bf16", "bf16->bf16")):
            ref = next(x for x in rows if x["leg"] == name and x["op"] == r["op"])
            r[key] = round(r["ms"] / ref["ms"], 3)
        print(json.dumps(r), flush=True)
    lines = [f"| {n}^2, {BLOCK}^2 blocks | op | ms (min .. max) | algorithmic GB/s | time / FLOAT | time / bf16 | check |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['leg']} | {r['op']} | {r['ms']} ({r['ms_min_max'][0]} .. {r['ms_min_max'][1]}) "
                     f"| {r['alg_gbs']} | {r['time_over_float']} | {r['time_over_bf16']} | {r['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
