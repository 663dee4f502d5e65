"""Mixed-precision transforms against "convert, then transform" on one GPU.

  (a) the fused mixed transform: A (its own type) -> C (another type) in one call;
  (b) what a caller did before: a torch copy_ of A into a preallocated temporary of C's type,
      then the same-type transform of the temporary.

Both run in one process on the same buffers.  Each is timed by device events on one stream around
`--reps` stream-ordered calls, after `--warmup` calls of each; the two alternate over `--rounds`
rounds and the medians of the per-call round means are reported with their spread (min .. max).
Before the timing, one call of each from the same C must give identical bits.

GB/s and the share of the 8 TB/s HBM peak are for (a), on its algorithmic bytes
n * (E_A + E_C [+ E_C when beta != 0]); the byte counts alone predict (a)/(b) = 12/20 for the
narrowing cases and 12/28 for the widening one (24/40 for c128 -> c64 with beta).

    python tools/bench_mixed.py [--reps 20] [--rounds 7] [--warmup 5] [--small] [--case K] [--out FILE]
Prints one JSON line per case and a markdown table; --small runs 2048^2 (a dry run of the script).
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

PEAK_GBS = 8000.0
TORCH = {costa.FLOAT: torch.float32, costa.DOUBLE: torch.float64, costa.CFLOAT: torch.complex64,
         costa.CDOUBLE: torch.complex128}
ESIZE = {costa.FLOAT: 4, costa.DOUBLE: 8, costa.CFLOAT: 8, costa.CDOUBLE: 16}
NAME = {costa.FLOAT: "f32", costa.DOUBLE: "f64", costa.CFLOAT: "c64", costa.CDOUBLE: "c128"}

# (n, block, A type, C type, op, alpha, beta)
CASES = [
    (16384, 256, costa.DOUBLE, costa.FLOAT, "T", 1, 0),
    (16384, 256, costa.DOUBLE, costa.FLOAT, "N", 1, 0),
    (16384, 256, costa.FLOAT, costa.DOUBLE, "T", 1, 0),
    (8192, 256, costa.CDOUBLE, costa.CFLOAT, "C", 0.75 - 0.5j, 1.25 + 0.25j),
]


def rand(n, dt, gen):
    if dt.is_complex:
        rt = torch.float32 if dt == torch.complex64 else torch.float64
        return torch.view_as_complex(torch.rand(n, 2, dtype=rt, device="cuda", generator=gen) * 2 - 1)
    return torch.rand(n, dtype=dt, device="cuda", generator=gen) * 2 - 1


def layout(n, b, t, code):
    return costa.block_cyclic_layout(n, n, b, b, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     code)


def run_case(n, b, ta, tc, op, alpha, beta, args, comm):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    A = rand(n * n, TORCH[ta], gen)
    C0 = rand(n * n, TORCH[tc], gen)
    C = C0.clone()
    tmp = torch.empty(n * n, dtype=TORCH[tc], device="cuda")
    LA, LC, LT = layout(n, b, A, ta), layout(n, b, C, tc), layout(n, b, tmp, tc)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()  # a stream of its own: the library joins it at entry and exit
    with torch.cuda.stream(s):
        return timed(n, b, ta, tc, op, alpha, beta, args, comm, s, A, C, C0, tmp, LA, LC, LT)


def timed(n, b, ta, tc, op, alpha, beta, args, comm, s, A, C, C0, tmp, LA, LC, LT):
    def fused():
        costa.transform_async(LA, LC, comm, op, alpha, beta, stream=s)

    def two_pass():
        tmp.copy_(A)
        costa.transform_async(LT, LC, comm, op, alpha, beta, stream=s)

    # identical bits, from the same C
    fused()
    s.synchronize()
    got_a = C.clone()
    C.copy_(C0)
    two_pass()
    s.synchronize()
    same = bool(torch.equal(got_a.view(torch.uint8), C.view(torch.uint8)))
    del got_a

    for f in (fused, two_pass):
        for _ in range(args.warmup):
            f()
    s.synchronize()
    ms = {"a": [], "b": []}
    for _ in range(args.rounds):
        for key, f in (("a", fused), ("b", two_pass)):
            C.copy_(C0)  # beta != 0: keep the values finite over many calls
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(args.reps):
                f()
            e1.record(s)
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / args.reps)
    a, bb = statistics.median(ms["a"]), statistics.median(ms["b"])
    nbytes = n * n * (ESIZE[ta] + ESIZE[tc] * (2 if beta else 1))
    gbs = nbytes / (a * 1e-3) / 1e9
    return {"case": f"{n}^2 {NAME[ta]}->{NAME[tc]} '{op}'" + (" alpha,beta" if beta else ""),
            "block": b, "identical_bits": same,
            "fused_ms": round(a, 4), "fused_ms_min_max": [round(min(ms["a"]), 4), round(max(ms["a"]), 4)],
            "two_pass_ms": round(bb, 4),
            "two_pass_ms_min_max": [round(min(ms["b"]), 4), round(max(ms["b"]), 4)],
            "ratio": round(a / bb, 3), "alg_bytes": nbytes, "fused_gbs": round(gbs, 1),
            "fused_share_of_peak": round(gbs / PEAK_GBS, 3), "reps": args.reps, "rounds": args.rounds}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--case", type=int, action="append",
                    help="run only this case (0-3; may be repeated), e.g. under a profiler")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mixed.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    rows = []
    for n, b, ta, tc, op, alpha, beta in [c for i, c in enumerate(CASES) if not args.case or i in args.case]:
        r = run_case(2048 if args.small else n, b, ta, tc, op, alpha, beta, args, comm)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    lines = ["| case | fused (a) ms | convert + transform (b) ms | (a)/(b) | (a) GB/s | of 8 TB/s | identical bits |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['fused_ms']} ({r['fused_ms_min_max'][0]} .. {r['fused_ms_min_max'][1]}) "
                     f"| {r['two_pass_ms']} ({r['two_pass_ms_min_max'][0]} .. {r['two_pass_ms_min_max'][1]}) "
                     f"| {r['ratio']} | {r['fused_gbs']} | {r['fused_share_of_peak']} | {r['identical_bits']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["identical_bits"] and r["ratio"] < 1 for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
