"""Scaled transforms against the ordinary transform of the same pair and geometry, and against the
two-pass alternative (a torch elementwise pass, then the ordinary transform), on one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), 'N' and 'T' with alpha, beta = 1, 0, both scale
vectors given:
    fp32 -> fp32, fp64 -> fp64, fp32 -> e4m3, e4m3 -> fp32, bf16 -> bf16      (scaled_kernels.hip)
Each leg is timed beside
    ordinary   costa.transform of the same pair and geometry (no scaling): scaled / ordinary is the
               figure of merit -- the fused call adds (m + n) scale elements of traffic
    two-pass   the scaling as torch elementwise multiplications `a * r[:, None] * c[None, :]` on the
               side that holds the compute type (into a temporary before the transform where A holds
               it, bf16 included; in place on C after it for e4m3 -> fp32), plus the ordinary transform
All run in one process, stream-ordered.  Each is timed by device events on one stream around `--reps`
calls, after `--warmup` calls of each; the legs alternate over `--rounds` rounds and the medians of
the per-call round means are reported with their spread.  Before the timing every scaled leg is
compared, bit for bit over the whole matrix, with torch's own arithmetic on the same data (two
rounded fp32 / fp64 products, one cast).

    python tools/bench_scaled.py [--reps 20] [--rounds 7] [--warmup 5] [--small] [--out FILE]
Prints one JSON line per leg and a markdown table; --small runs 2048^2 (a dry run of the script).
COSTA_TUNING=1 COSTA_SCALED_ORDER=0 runs the scaled LOCAL list in list order instead of
destination-address order.
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
    ("fp32->fp32", torch.float32, torch.float32),
    ("fp64->fp64", torch.float64, torch.float64),
    ("fp32->e4m3", torch.float32, Q),
    ("e4m3->fp32", Q, torch.float32),
    ("bf16->bf16", torch.bfloat16, torch.bfloat16),
]
BLOCK = 256


def layout(n, t):
    return costa.block_cyclic_layout(n, n, BLOCK, BLOCK, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     costa.element_code(t.dtype))


def zeros(n, dt):
    return torch.zeros(n * n, dtype=torch.uint8, device="cuda").view(dt) if dt == Q \
        else torch.zeros(n * n, dtype=dt, device="cuda")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scaled.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    n = 2048 if args.small else 16384
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    base = torch.rand(n * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1
    src = {Q: base.cpu().to(Q).cuda(), torch.bfloat16: base.to(torch.bfloat16), torch.float32: base,
           torch.float64: base.to(torch.float64)}
    dst = {dt: zeros(n, dt) for dt in src}
    del base
    # scales with |v| in [0.5, 2), mixed sign
    rc = {}
    for ct in (torch.float32, torch.float64):
        v = (torch.rand(2 * n, dtype=torch.float64, device="cuda", generator=gen) * 1.49 + 0.5)
        v = v * (torch.randint(0, 2, (2 * n,), device="cuda", generator=gen) * 2 - 1)
        rc[ct] = (v[:n].to(ct).contiguous(), v[n:].to(ct).contiguous())
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    legs = []
    with torch.cuda.stream(s):
        for name, ta, tc in LEGS:
            A, C = src[ta], dst[tc]
            LA, LC = layout(n, A), layout(n, C)
            ct = torch.float64 if tc == torch.float64 else torch.float32
            r, c = rc[ct]
            a_holds_ct = ta != Q
            tmp = zeros(n, ta) if a_holds_ct else None
            LT = layout(n, tmp) if a_holds_ct else None
            for op in ("N", "T"):
                # column-major storage: view(n, n)[j, i] is element (i, j).  Target (i, j) takes
                # r[i] * c[j]; seen from A's view that is r along its last index for 'N', its first for 'T'
                Av, Cv = A.view(n, n), C.view(n, n)
                a_first, a_last = (c, r) if op == "N" else (r, c)

                def scaled(LA=LA, LC=LC, op=op, r=r, c=c):
                    costa.transform_scaled(LA, LC, comm, op, 1, 0, r, c, stream=s)

                def ordinary(LA=LA, LC=LC, op=op):
                    costa.transform_async(LA, LC, comm, op, 1, 0, stream=s)

                if a_holds_ct:
                    def two_pass(Av=Av, tmp=tmp, LT=LT, LC=LC, op=op, a_first=a_first, a_last=a_last):
                        tv = tmp.view(n, n)
                        torch.mul(Av, a_last[None, :] if op == "N" else a_first[:, None], out=tv)
                        torch.mul(tv, a_first[:, None] if op == "N" else a_last[None, :], out=tv)
                        costa.transform_async(LT, LC, comm, op, 1, 0, stream=s)
                else:
                    def two_pass(LA=LA, LC=LC, Cv=Cv, op=op, r=r, c=c):
                        costa.transform_async(LA, LC, comm, op, 1, 0, stream=s)
                        Cv.mul_(r[None, :])
                        Cv.mul_(c[:, None])
                # whole-matrix check of the scaled leg against torch's arithmetic: (w(a) * r) * c in
                # the compute type, r first, then one cast (FLOAT -> e4m3: torch-CPU's conversion,
                # the one the library is pinned to)
                C.view(torch.uint8).zero_()
                scaled()
                s.synchronize()
                w = (Av.to(ct).transpose(0, 1) if op == "T" else Av.to(ct))
                want = (w * r[None, :]) * c[:, None]
                del w
                want = want.cpu().to(Q).cuda() if tc == Q else want.to(tc)
                same = bool(torch.equal(want.contiguous().view(-1).view(torch.uint8), C.view(torch.uint8)))
                del want
                for variant, call in (("scaled", scaled), ("ordinary", ordinary), ("two-pass", two_pass)):
                    legs.append({"leg": name, "op": op, "variant": variant, "call": call,
                                 "check_passed": same if variant == "scaled" else None,
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
    lines = [f"| {n}^2, {BLOCK}^2 blocks | op | scaled ms (min .. max) | GB/s | ordinary ms | two-pass ms | "
             "scaled / ordinary | scaled / two-pass | check |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, _, _ in LEGS:
        for op in ("N", "T"):
            g = {r["variant"]: r for r in rows if r["leg"] == name and r["op"] == op}
            sc, od, tp = g["scaled"], g["ordinary"], g["two-pass"]
            lines.append(f"| {name} | {op} | {sc['ms']} ({sc['ms_min_max'][0]} .. {sc['ms_min_max'][1]}) "
                         f"| {sc['alg_gbs']} | {od['ms']} | {tp['ms']} | {sc['ms'] / od['ms']:.3f} "
                         f"| {sc['ms'] / tp['ms']:.3f} | {sc['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
