"""amax outputs against the scaled transform of the same pair and geometry, against the two-pass
alternative, and the reduce-only pass against torch's reductions, on one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), 'N' and 'T' with alpha, beta = 1, 0, both scale
vectors given:
    fp32 -> fp32, fp64 -> fp64, fp32 -> e4m3, e4m3 -> fp32, bf16 -> bf16      (scaled_kernels.hip)
Each leg is timed as
    amax        costa.transform_amax with both amax vectors, which are zeroed before every call (two
                torch fills inside the timed region: a vector already at its maxima would let the
                kernel skip every atomic)
    scaled      costa.transform_scaled of the same library: amax / scaled is the figure of merit
    two-pass    torch `abs().amax()` of A over both dimensions (an e4m3 source is widened to fp32
                first: torch reduces no FP8), then costa.transform_scaled
    layout      costa.layout_amax of A with both vectors (zeroed before every call)
    torch-amax  the two torch reductions alone
All run in one process, stream-ordered, timed by device events on one stream around `--reps` calls
after `--warmup` calls of each; the legs alternate over `--rounds` rounds and the medians of the
per-call round means are reported with their spread.  Before the timing every amax leg is compared
with torch on the same data: C bit for bit over the whole matrix (two rounded products, one cast),
the vectors bit for bit with torch's `abs().amax()` of the widened source.

    python tools/bench_amax.py [--reps 20] [--rounds 7] [--warmup 5] [--small] [--scaled-only] [--pad-mib N] [--out FILE]
Prints one JSON line per leg and a markdown table; --small runs 2048^2 (a dry run of the script).
--scaled-only times only `scaled` (a library without the amax entry points, selected with COSTA_LIB:
the yardstick for "nothing existing got slower"); --pad-mib N allocates N MiB ahead of every buffer.
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
    ap.add_argument("--scaled-only", action="store_true")
    ap.add_argument("--pad-mib", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_amax.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    n = 2048 if args.small else 16384
    # (an allocation ahead of all others moves every buffer: how much of a difference between two
    # libraries is the placement of the data)
    pad = torch.zeros(args.pad_mib << 20, dtype=torch.uint8, device="cuda") if args.pad_mib else None  # noqa: F841
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    base = torch.rand(n * n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1
    src = {Q: base.cpu().to(Q).cuda(), torch.bfloat16: base.to(torch.bfloat16), torch.float32: base,
           torch.float64: base.to(torch.float64)}
    dst = {dt: zeros(n, dt) for dt in src}
    del base
    rc, amx = {}, {}
    for ct in (torch.float32, torch.float64):
        v = (torch.rand(2 * n, dtype=torch.float64, device="cuda", generator=gen) * 1.49 + 0.5)
        v = v * (torch.randint(0, 2, (2 * n,), device="cuda", generator=gen) * 2 - 1)
        rc[ct] = (v[:n].to(ct).contiguous(), v[n:].to(ct).contiguous())
        amx[ct] = (torch.zeros(n, dtype=ct, device="cuda"), torch.zeros(n, dtype=ct, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    legs = []
    with torch.cuda.stream(s):
        for name, ta, tc in LEGS:
            A, C = src[ta], dst[tc]
            LA, LC = layout(n, A), layout(n, C)
            ct = torch.float64 if tc == torch.float64 else torch.float32
            lt = torch.float64 if ta == torch.float64 else torch.float32  # layout_amax's vector type
            r, c = rc[ct]
            ra, ca = amx[ct]
            la_r, la_c = amx[lt]
            for op in ("N", "T"):
                # column-major storage: view(n, n)[j, i] is element (i, j) of A; target row i of 'N'
                # collects A's row i = dim 0 of the view reduced away, of 'T' A's column i = dim 1
                Av = A.view(n, n)
                rdim, cdim = (0, 1) if op == "N" else (1, 0)

                def scaled(LA=LA, LC=LC, op=op, r=r, c=c):
                    costa.transform_scaled(LA, LC, comm, op, 1, 0, r, c, stream=s)

                def fused(LA=LA, LC=LC, op=op, r=r, c=c, ra=ra, ca=ca):
                    ra.zero_()
                    ca.zero_()
                    costa.transform_amax(LA, LC, comm, op, 1, 0, r, c, ra, ca, stream=s)

                def torch_amax(Av=Av, rdim=rdim, cdim=cdim):
                    w = Av.to(torch.float32) if Av.dtype == Q else Av
                    return w.abs().amax(dim=rdim), w.abs().amax(dim=cdim)

                def two_pass(LA=LA, LC=LC, op=op, r=r, c=c, torch_amax=torch_amax):
                    torch_amax()
                    costa.transform_scaled(LA, LC, comm, op, 1, 0, r, c, stream=s)

                def layout_amax(LA=LA, la_r=la_r, la_c=la_c):
                    la_r.zero_()
                    la_c.zero_()
                    costa.layout_amax(LA, comm, la_r, la_c, stream=s)

                same = None
                if not args.scaled_only:
                    # C against torch's arithmetic, (w(a) * r) * c in the compute type, r first, one
                    # cast (FLOAT -> e4m3: torch-CPU's conversion); the vectors against torch's amax
                    C.view(torch.uint8).zero_()
                    fused()
                    s.synchronize()
                    w = (Av.to(ct).transpose(0, 1) if op == "T" else Av.to(ct))
                    want = (w * r[None, :]) * c[:, None]
                    del w
                    want = want.cpu().to(Q).cuda() if tc == Q else want.to(tc)
                    same = bool(torch.equal(want.contiguous().view(-1).view(torch.uint8), C.view(torch.uint8)))
                    del want
                    tr, tcl = torch_amax()
                    same = same and bool(torch.equal(tr.to(ct), ra)) and bool(torch.equal(tcl.to(ct), ca))
                    if op == "N":  # the layout's own rows and columns
                        layout_amax()
                        s.synchronize()
                        same = same and bool(torch.equal(tr.to(lt), la_r)) and bool(torch.equal(tcl.to(lt), la_c))
                variants = [("scaled", scaled)]
                if not args.scaled_only:
                    variants += [("amax", fused), ("two-pass", two_pass)]
                    if op == "N":
                        variants += [("layout", layout_amax), ("torch-amax", torch_amax)]
                for variant, call in variants:
                    legs.append({"leg": name, "op": op, "variant": variant, "call": call,
                                 "check_passed": same if variant == "amax" else None, "ms": []})
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
                     "reps": args.reps, "rounds": args.rounds, "lib": os.environ.get("COSTA_LIB", "")})
    for r in rows:
        print(json.dumps(r), flush=True)
    lines = []
    if args.scaled_only:
        lines += [f"| {n}^2, {BLOCK}^2 blocks | op | scaled ms (min .. max) |", "|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['leg']} | {r['op']} | {r['ms']} ({r['ms_min_max'][0]} .. {r['ms_min_max'][1]}) |")
    else:
        lines += [f"| {n}^2, {BLOCK}^2 blocks | op | amax ms (min .. max) | scaled ms (min .. max) | two-pass ms | "
                  "amax / scaled | amax / two-pass | layout ms | torch-amax ms | check |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for name, _, _ in LEGS:
            for op in ("N", "T"):
                g = {r["variant"]: r for r in rows if r["leg"] == name and r["op"] == op}
                am, sc, tp = g["amax"], g["scaled"], g["two-pass"]
                la = g["layout"]["ms"] if "layout" in g else ""
                to = g["torch-amax"]["ms"] if "torch-amax" in g else ""
                lines.append(f"| {name} | {op} | {am['ms']} ({am['ms_min_max'][0]} .. {am['ms_min_max'][1]}) "
                             f"| {sc['ms']} ({sc['ms_min_max'][0]} .. {sc['ms_min_max'][1]}) | {tp['ms']} "
                             f"| {am['ms'] / sc['ms']:.3f} | {am['ms'] / tp['ms']:.3f} | {la} | {to} "
                             f"| {am['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
