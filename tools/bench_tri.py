"""Triangular (masked) transforms against the full transform of the same geometry on one GPU.

  (a) transform_tri: only the tiles inside the mask move, the tiles the diagonal cuts through the
      edge-tile kernel;
  (b) the full transform of the same layouts.

Both run in one process on the same buffers, stream-ordered as the headline benchmark does.  Each is
timed by device events on one stream around `--reps` calls, after `--warmup` calls of each; the two
alternate over `--rounds` rounds and the medians of the per-call round means are reported with
their spread (min .. max).  Before the timing, one masked call must give, over the full matrix,
torch.where(mask, full result, C before) bit for bit.

Cases: 16384^2 fp64 in 256^2 blocks, 'N' 'U' k = 0; the same pair 'T' 'L' k = -1 with alpha, beta;
an 8192^2 single-block custom layout 'N' 'U' (the planner's band cut).  For each: both times, the
ratio of the algorithmic bytes (masked / full, from the library's counters) and tri_items; with
--phases also the LOCAL phase times of both calls from the library's phase events and the edge-tile
launch's share of the masked call.

    python tools/bench_tri.py [--reps 20] [--rounds 7] [--warmup 5] [--small] [--case K] [--out FILE]
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

# (n, block or None for one custom block, op, uplo, k, alpha, beta)
CASES = [
    (16384, 256, "N", "U", 0, 1, 0),
    (16384, 256, "T", "L", -1, 0.75, -1.5),
    (8192, None, "N", "U", 0, 1, 0),
]


def layout(n, b, t):
    if b is None:
        return costa.custom_layout(1, 1, [0, n], [0, n], [0], [(t.data_ptr(), n, 0, 0)], "C", costa.DOUBLE)
    return costa.block_cyclic_layout(n, n, b, b, 1, 1, n, n, 1, 1, "R", 0, 0, t.data_ptr(), n, "C", 0,
                                     costa.DOUBLE)


def run_case(n, b, op, uplo, k, alpha, beta, args, comm):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    A = torch.rand(n * n, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    C0 = torch.rand(n * n, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    C = C0.clone()
    LA, LC = layout(n, b, A), layout(n, b, C)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        return timed(n, b, op, uplo, k, alpha, beta, args, comm, s, A, C, C0, LA, LC)


def timed(n, b, op, uplo, k, alpha, beta, args, comm, s, A, C, C0, LA, LC):
    def masked():
        costa.transform_tri_async(LA, LC, comm, op, uplo, k, alpha, beta, stream=s)

    def full():
        costa.transform_async(LA, LC, comm, op, alpha, beta, stream=s)

    # full-matrix check: where(mask, full result, C before), bit for bit (column-major storage:
    # element (i, j) at j * n + i, i.e. the torch view [j, i])
    st0 = costa.get_stats()
    full()
    s.synchronize()
    st1 = costa.get_stats()
    c_full = C.clone()
    C.copy_(C0)
    masked()
    s.synchronize()
    st2 = costa.get_stats()
    j = torch.arange(n, device="cuda").view(n, 1)
    i = torch.arange(n, device="cuda").view(1, n)
    keep = (j - i >= k) if uplo == "U" else (j - i <= k)
    want = torch.where(keep, c_full.view(n, n), C0.view(n, n))
    same = bool(torch.equal(want.view(torch.uint8), C.view(n, n).view(torch.uint8)))
    del c_full, want, keep
    bytes_full = st1["local_bytes"] - st0["local_bytes"]
    bytes_masked = st2["local_bytes"] - st1["local_bytes"]
    tri_items = st2["tri_items"] - st1["tri_items"]

    for f in (masked, full):
        for _ in range(args.warmup):
            f()
    s.synchronize()
    ms = {"a": [], "b": []}
    for _ in range(args.rounds):
        for key, f in (("a", masked), ("b", full)):
            C.copy_(C0)  # beta != 0: keep the values finite over many calls
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(args.reps):
                f()
            e1.record(s)
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / args.reps)
    a, bb = statistics.median(ms["a"]), statistics.median(ms["b"])
    gbs = bytes_masked / (a * 1e-3) / 1e9
    name = f"{n}^2 f64 " + (f"{b}^2 blocks" if b else "one block") + f" '{op}' '{uplo}' k={k}"
    return {"case": name + (" alpha,beta" if beta else ""), "check_passed": same,
            "masked_ms": round(a, 4), "masked_ms_min_max": [round(min(ms["a"]), 4), round(max(ms["a"]), 4)],
            "full_ms": round(bb, 4), "full_ms_min_max": [round(min(ms["b"]), 4), round(max(ms["b"]), 4)],
            "time_ratio": round(a / bb, 3), "byte_ratio": round(bytes_masked / bytes_full, 3),
            "time_over_byte_ratio": round((a / bb) / (bytes_masked / bytes_full), 3),
            "alg_bytes_masked": bytes_masked, "alg_bytes_full": bytes_full, "masked_gbs": round(gbs, 1),
            "tri_items": tri_items, "reps": args.reps, "rounds": args.rounds}


def phase_split(n, b, op, uplo, k, alpha, beta, comm, reps=10):
    """Where the masked call's time goes, from the library's phase events (profiling on, blocking
    calls, a pass of its own): LOCAL ms per call of the masked and of the full transform, and of
    the masked call's LOCAL time the part its edge-tile launch takes (tri_phase_ms); the rest is
    the ordinary launch over the wholly kept tiles."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    A = torch.rand(n * n, dtype=torch.float64, device="cuda", generator=gen)
    C = torch.rand(n * n, dtype=torch.float64, device="cuda", generator=gen)
    LA, LC = layout(n, b, A), layout(n, b, C)

    def local_ms(f):
        for _ in range(3):
            f()
        costa.set_profiling(True)
        costa.get_stats(reset=True)
        costa.tri_phase_ms(reset=True)
        for _ in range(reps):
            f()
        st = costa.get_stats(reset=True)
        edge = costa.tri_phase_ms(reset=True)
        costa.set_profiling(False)
        return st["local_ms"] / reps, edge / reps, st["local_bytes"] // reps
    m_ms, e_ms, m_bytes = local_ms(lambda: costa.transform_tri(LA, LC, comm, op, uplo, k, alpha, beta))
    f_ms, _, f_bytes = local_ms(lambda: costa.transform(LA, LC, comm, op, alpha, beta))
    p = costa.plan_export_tri(LA, LC, 0, 1, op, uplo, k, alpha, beta)
    per_elem = 8 * (3 if beta else 2)
    ordinary_bytes = int((p.local_ops["nf"].astype("int64") * p.local_ops["ns"]).sum()) * per_elem
    o_ms = m_ms - e_ms
    return {"masked_local_ms": round(m_ms, 4), "edge_launch_ms": round(e_ms, 4),
            "edge_launch_share": round(e_ms / m_ms, 3), "ordinary_launch_ms": round(o_ms, 4),
            "ordinary_tiles_bytes": ordinary_bytes, "edge_tiles_kept_bytes": int(m_bytes - ordinary_bytes),
            "ordinary_launch_gbs": round(ordinary_bytes / (o_ms * 1e-3) / 1e9, 1),
            "edge_launch_kept_gbs": round((m_bytes - ordinary_bytes) / (e_ms * 1e-3) / 1e9, 1) if e_ms else None,
            "full_local_ms": round(f_ms, 4), "full_gbs": round(f_bytes / (f_ms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--case", type=int, action="append", help="run only this case (0-2; may be repeated)")
    ap.add_argument("--phases", action="store_true", help="also the LOCAL phase split of each case")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tri.py needs a GPU (there is no CPU path to time)")
    torch.cuda.set_device(0)
    comm = costa.Comm.self(0)
    rows = []
    for n, b, op, uplo, k, alpha, beta in [c for i, c in enumerate(CASES) if not args.case or i in args.case]:
        n = 2048 if args.small else n
        r = run_case(n, b, op, uplo, k, alpha, beta, args, comm)
        if args.phases:
            r["phases"] = phase_split(n, b, op, uplo, k, alpha, beta, comm)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    lines = ["| case | masked ms | full ms | time ratio | byte ratio | time / byte | tri_items | check |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['masked_ms']} ({r['masked_ms_min_max'][0]} .. {r['masked_ms_min_max'][1]}) "
                     f"| {r['full_ms']} ({r['full_ms_min_max'][0]} .. {r['full_ms_min_max'][1]}) "
                     f"| {r['time_ratio']} | {r['byte_ratio']} | {r['time_over_byte_ratio']} "
                     f"| {r['tri_items']} | {r['check_passed']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] and r["time_ratio"] < 1 for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
