"""Stochastic-rounding legs of transform_mx beside the round-to-nearest legs of the same geometry, on
one GPU.

One rank, n x n in 256 x 256 blocks (n = 16384), beta = 0, rounding floor.  Legs, for Q = e4m3 and Q =
packed e2m1:
    quantise 'N', 'T'        fp32 -> Q, blocks of C along rows, alpha = 1
    requantise 'T' r->c      Q (blocks along A's rows) -> Q (blocks along C's columns), alpha = 0.625
    requantise 'T' c->c      Q (blocks along A's columns) -> Q (blocks along C's columns), alpha = 0.625
each once with `stochastic_seed` (the SR instance of mx_kernel: the code under test) and once without
(the round-to-nearest instance: the reference, unchanged code).  alpha = 0.625 on the requantise legs
makes most products fall between two codes, so the SR legs have something to decide.

All legs run in one process, stream-ordered, timed by device events around `--reps` calls after
`--warmup` calls of each; an SR leg and its plain leg follow each other inside every one of `--rounds`
rounds, and the medians of the per-call round means are reported with their min .. max, the ratio
SR / plain per round likewise.  Before the timing every SR leg is compared, bit for bit over the whole
matrix and the whole scale tensor, with the arithmetic of costa_hip.h, "Stochastic rounding in the MX
transforms", written in torch on the GPU: the hash in 64-bit integers masked to 32 bits, the conversion
from the type's table of magnitudes (lo / hi search, T = floor((a - lo) / (hi - lo) * 2^24) in float64),
independent of the kernel's integer routine.

    python tools/bench_mx_sr.py [--reps 10] [--rounds 5] [--warmup 3] [--small] [--out FILE]
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
TYPE = {Q8: dict(emax=8, fmax=448.0, sign=0x80, shift=24), Q4: dict(emax=2, fmax=6.0, sign=8, shift=28)}
BLOCK = 256
ROWS, COLS = costa.MX_ROWS, costa.MX_COLS
SEED = 0x0123456789ABCDEF
M32, M24 = 0xFFFFFFFF, 1 << 24
CHUNK = 1024  # stored lines of C converted at a time by the check
# (name, A is Q, op, a_axis, c_axis, alpha)
LEGS = [
    ("quantise", False, "N", None, ROWS, 1.0),
    ("quantise", False, "T", None, ROWS, 1.0),
    ("requantise r->c", True, "T", ROWS, COLS, 0.625),
    ("requantise c->c", True, "T", COLS, COLS, 0.625),
]


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


def pow2(e):
    return (e.to(torch.int32) << 23).view(torch.float32)


def magnitudes(q):
    """the finite magnitudes of the type in code order, from the format's definition"""
    if q == Q4:
        return [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    return [m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7) for e in range(16) for m in range(8)][:127]


def widen(packed, n, q):
    """Q bytes (column-major; e2m1: rows share bytes, the even row in the low half) -> fp32 view(n, n)"""
    mags = magnitudes(q)
    if q == Q8:
        mags = mags + [float("nan")]
        codes = packed.view(n, n)
    else:
        b = packed.view(n, n // 2)
        codes = torch.stack((b & 15, b >> 4), dim=2).view(n, n)
    lut = torch.tensor(mags + [-x for x in mags], dtype=torch.float32, device="cuda")
    return lut[codes.to(torch.int64)]


def fmix32(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def host_fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def rand24(seed, n, j0, j1):
    """U(seed, i, j) for the stored lines j0 .. j1 - 1 of C: [j - j0, i], int64"""
    k0 = host_fmix32((seed & M32) ^ 0x9E3779B9)
    k1 = host_fmix32((seed >> 32) ^ 0x85EBCA6B)
    i = torch.arange(n, dtype=torch.int64, device="cuda").unsqueeze(0)
    j = torch.arange(j0, j1, dtype=torch.int64, device="cuda").unsqueeze(1)
    return fmix32(((fmix32(i ^ k0) + j) & M32) ^ k1) >> 8


def sr_bytes(t, U, q):
    """clamped t [lines, n] and its random bits -> the stored bytes of those lines"""
    mags = torch.tensor(magnitudes(q), dtype=torch.float64, device="cuda")
    a = t.abs().to(torch.float64)
    k = torch.bucketize(a, mags, right=True) - 1
    lo, hi = mags[k], mags[(k + 1).clamp_(max=mags.numel() - 1)]
    T = torch.where(hi > lo, torch.floor((a - lo) / (hi - lo) * M24), torch.zeros_like(a)).to(torch.int64)
    code = k + (T + U >= M24).to(torch.int64)
    code |= (t.view(torch.int32).to(torch.int64) >> TYPE[q]["shift"]) & TYPE[q]["sign"]
    code = code.to(torch.uint8)
    if q == Q8:
        return code.reshape(-1)
    c = code.view(code.shape[0], -1, 2)
    return (c[:, :, 0] | c[:, :, 1] << 4).reshape(-1)


def model(n, op, src, q, a_q, SA, a_axis, c_axis, alpha, seed, sc_out):
    """the expected destination bytes of an SR leg (and sc_out filled), in torch on the GPU"""
    x = widen(src, n, q) if a_q else src.view(n, n)
    if a_q:
        b = x.view(n, n // 32, 32) if a_axis == ROWS else x.view(n // 32, 32, n)
        x = (b * pow2(SA).unsqueeze(2 if a_axis == ROWS else 1)).view(n, n)
    if alpha != 1.0:
        x = x * alpha
    out = torch.empty(nbytes(n, q), dtype=torch.uint8, device="cuda")
    per_line = nbytes(n, q) // n
    fm, emax = TYPE[q]["fmax"], TYPE[q]["emax"]
    for j0 in range(0, n, CHUNK):
        j1 = min(n, j0 + CHUNK)
        v = (x[:, j0:j1].T if op == "T" else x[j0:j1, :]).contiguous()     # [line j, row i]
        if c_axis == ROWS:
            b, d = v.view(j1 - j0, n // 32, 32), 2
        else:
            b, d = v.view((j1 - j0) // 32, 32, n), 1
        E = ((b.abs().amax(dim=d).view(torch.int32) >> 23) - emax).clamp_(0, 254)
        if c_axis == ROWS:
            sc_out[j0:j1, :] = E.to(torch.uint8)
        else:
            sc_out[j0 // 32:j1 // 32, :] = E.to(torch.uint8)
        t = (b * pow2(254 - E).unsqueeze(d)).clamp_(-fm, fm).view(j1 - j0, n)
        out[j0 * per_line:j1 * per_line] = sr_bytes(t, rand24(seed, n, j0, j1), q)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mx_sr.py needs a GPU (there is no CPU path to time)")
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
    dst = {kind: torch.zeros(nbytes(n, kind), dtype=torch.uint8, device="cuda") for kind in (Q8, Q4)}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    legs = []
    with torch.cuda.stream(s):
        for name, a_q, op, a_axis, c_axis, alpha in LEGS:
            rnd = lambda shape: torch.randint(120, 134, shape, dtype=torch.uint8, device="cuda", generator=gen)  # noqa: E731
            SA = scale_tensor(n, a_axis, rnd) if a_axis is not None else None
            for q in (Q8, Q4):
                ta = q if a_q else F
                A, C = src[ta], dst[q]
                LA, LC = layout(n, A, ta), layout(n, C, q)
                SC = scale_tensor(n, c_axis)
                da = descriptor(SA, a_axis) if SA is not None else None
                dc = descriptor(SC, c_axis)
                for variant, seed in (("sr", SEED), ("plain", None)):

                    def call(LA=LA, LC=LC, op=op, da=da, dc=dc, alpha=alpha, seed=seed):
                        costa.transform_mx(LA, LC, comm, op, alpha, 0.0, a_scales=da, c_scales=dc, stream=s,
                                           stochastic_seed=seed)

                    same = None
                    if seed is not None:  # whole-matrix check of the SR leg
                        SC2 = scale_tensor(n, c_axis)
                        C.zero_()
                        call()
                        s.synchronize()
                        want = model(n, op, A, q, a_q, SA, a_axis, c_axis, alpha, seed, SC2)
                        same = bool(torch.equal(want, C)) and bool(torch.equal(SC, SC2))
                        del want
                    legs.append({"leg": name, "op": op, "type": q, "variant": variant, "call": call,
                                 "check_passed": same, "bytes": nbytes(n, ta) + nbytes(n, q), "ms": []})
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
        rows.append({"leg": leg["leg"], "op": leg["op"], "type": leg["type"], "variant": leg["variant"], "n": n,
                     "block": BLOCK, "check_passed": leg["check_passed"], "ms": round(ms, 4),
                     "ms_min_max": [round(min(leg["ms"]), 4), round(max(leg["ms"]), 4)], "ms_rounds": leg["ms"],
                     "alg_bytes": leg["bytes"], "alg_gbs": round(leg["bytes"] / (ms * 1e-3) / 1e9, 1),
                     "reps": args.reps, "rounds": args.rounds})

    def cell(r):
        return f"{r['ms']} ({r['ms_min_max'][0]} .. {r['ms_min_max'][1]}) | {r['alg_gbs']}"
    lines = [f"| {n}^2, {BLOCK}^2 blocks | op | type | SR ms (min .. max) | GB/s | plain ms (min .. max) | GB/s | "
             "SR / plain (min .. max over rounds) | check |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, _, op, _, _, _ in LEGS:
        for q in (Q8, Q4):
            g = {r["variant"]: r for r in rows if r["leg"] == name and r["op"] == op and r["type"] == q}
            a, b = g["sr"], g["plain"]
            ratios = [x / y for x, y in zip(a["ms_rounds"], b["ms_rounds"])]
            a["sr_over_plain"] = round(a["ms"] / b["ms"], 3)
            a["sr_over_plain_min_max"] = [round(min(ratios), 3), round(max(ratios), 3)]
            lines.append(f"| {name} | {op} | {q} | {cell(a)} | {cell(b)} | {a['ms'] / b['ms']:.3f} "
                         f"({min(ratios):.3f} .. {max(ratios):.3f}) | {a['check_passed']} |")
    for r in rows:
        r["ms_rounds"] = [round(x, 4) for x in r["ms_rounds"]]
        print(json.dumps(r), flush=True)
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")
    return 0 if all(r["check_passed"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
