"""The tile-op lists of tests/test_gpu_tiles.py, by name, with the launches each one exists for.

tile_kernels.hip launch_t picks a kernel per work class from the split engine.cpp build_work made of
the list (merging, VEC-flag gains, granule cuts, class thresholds, kMinMediumOps, the square / 32 x 32
/ skew / group rules, the `full` flags).  `variants()` mirrors that choice from
costa_amd.work_export(...).meta on the host; every list in `LISTS` declares the launches it is there
to exercise, and the tests assert declared <= variants() before any kernel runs, so a dispatch rule
that moves fails the list that relied on it instead of silently retargeting it.

A builder returns (rng, code, ops, n_src, n_dst): TILE_OP_DTYPE ops with offsets relative to the
two buffers and the buffers' element counts (guard elements after the last op included); `build`
then draws the source elements, the destination's initial elements and the (alpha, beta) slot pairs
from the same generator (`ops_of` stops at the ops: all a route check needs).  Builders are
deterministic (seeded).

Variant names (an aliased launch is named as the kernel it aliases, so two names never mean one
kernel): large, large_tr, large_tr_full, small_tr, medium_tr, medium_tr_full, small32_tr, skew,
skew_wide, cblock_{N,T}[ax][+pieces], tiny_{N,T}[ax].
"""
import functools

import numpy as np

import costa_amd
import oracle
import specials_common

TINY_LDS = 4096  # engine.hpp kTinyLdsDefault
CODES = {"f32": 0, "f64": 1, "c64": 2, "c128": 3, "i32": 4}
NAMES = {v: k for k, v in CODES.items()}
REAL = ("f32", "f64", "i32")  # engine.cpp cblock_enabled / tile_kernels.hip launch_skew

TR, CONJ, VEC_SRC, VEC_DST = 1, 2, 4, 8
AXPBY = 3


def tiny_copy(E, local=True):
    """engine.cpp tiny_copy_budget: half a wavefront pass for local lists (32 lanes x
    tiny_copy_lane_bytes), 3/4 for pack / unpack lists (48 lanes)"""
    return (32 if local else 48) * 64


def group_budget(E):
    """engine.cpp build_work group_budget: the largest leading dimension a destination-block group
    may write (cblock_max_elems(E) - (16 / E - 1), engine.hpp kCblockThreads x kCblockChunks vectors)"""
    return 256 * 4 * (16 // E) - (16 // E - 1)


# ---------------------------------------------------------------------------- routes
# the launch a name of tile_kernels.hip shapes<T> really is, where it is an alias there
_ALIAS = {
    "f32": {"large_tr_full": "large_tr"},                                # shapes<float>
    "i32": {"large_tr_full": "large_tr"},                                # shapes<int>
    "f64": {"large_tr_full": "large_tr", "medium_tr_full": "medium_tr"},  # shapes<double>
    "c64": {"large_tr_full": "large_tr"},                                # shapes<cpx<float>>
    "c128": {},                                                          # shapes<cpx<double>>
}
_HAS_SMALL = {"f64", "c64", "c128"}   # shapes<T>::has_small
_HAS_MEDIUM = {"f32", "f64", "i32"}   # shapes<T>::has_medium


def split(dtype, ops, kind="local"):
    """work_export's meta with the flag bits named (costa_hip_work_export, capi.cpp)"""
    m = dict(costa_amd.work_export(dtype, ops, kind).meta)
    for bit, name in enumerate(("tr_shape", "sq", "full", "med_full", "med_sq", "skew_wide")):
        m[name] = bool(m["flags"] >> bit & 1)
    return m


def variants(dtype, ops, kind="local"):
    """the launches tile_kernels.hip launch_t issues for this list (host builder, no kernel runs)"""
    t = NAMES[int(dtype)]
    m = split(dtype, ops, kind)
    fl = np.asarray(ops["flags"], np.uint32)
    any_tr = bool((fl & TR).any())                      # engine.cpp any_transpose
    any_ax = bool(((fl >> 4 & 3) == AXPBY).any())       # engine.cpp any_axpby
    alias = _ALIAS[t]
    out = set()
    # launch_t: the large class
    if m["n_large"] > 0:
        if m["sq"]:
            if t not in _HAS_SMALL or not m["tr_shape"]:
                raise AssertionError("launch_t would throw: square shape")
            v = "small_tr"
        elif m["tr_shape"] and m["full"]:
            v = "large_tr_full"
        elif m["tr_shape"]:
            v = "large_tr"
        else:
            v = "large"
        out.add(alias.get(v, v))
    # the medium class
    if m["n_medium"] > 0 and m["med_sq"]:
        if not m["tr_shape"]:
            raise AssertionError("launch_t would throw: 32 x 32 shape")
        out.add("small32_tr")
    elif m["n_medium"] > 0:
        if t not in _HAS_MEDIUM or not m["tr_shape"]:
            raise AssertionError("launch_t would throw: medium shape")
        v = "medium_tr_full" if m["med_full"] and not any_ax else "medium_tr"
        out.add(alias.get(v, v))
    # launch_skew
    if m["n_skew"] > 0:
        if t not in REAL:
            raise AssertionError("launch_skew would throw: complex type")
        out.add("skew_wide" if m["skew_wide"] and t in ("f32", "i32") else "skew")
    # launch_cblock / launch_tiny (pieces_in_group_launch: fused when both exist, real types)
    suffix = ("T" if any_tr else "N") + ("ax" if any_ax else "")
    fuse = t in REAL and m["n_cblock"] > 0 and m["n_tiny"] > 0
    if m["n_cblock"] > 0:
        if t not in REAL:
            raise AssertionError("launch_cblock would throw: complex type")
        out.add("cblock_" + suffix + ("+pieces" if fuse else ""))
    if m["n_tiny"] > 0 and not fuse:
        out.add("tiny_" + suffix)
    return out


# sub-tile (BF, BS) of each tile_kernel launch, by hand from tile_kernels.hip shapes<T>
_DIMS = {
    "f32": {"large": (256, 16), "large_tr": (128, 128), "medium_tr": (64, 64), "medium_tr_full": (64, 64),
            "small32_tr": (32, 32)},
    "i32": {"large": (256, 16), "large_tr": (128, 128), "medium_tr": (64, 64), "medium_tr_full": (64, 64),
            "small32_tr": (32, 32)},
    "f64": {"large": (128, 16), "large_tr": (64, 128), "small_tr": (64, 64), "medium_tr": (32, 64),
            "small32_tr": (32, 32)},
    "c64": {"large": (128, 16), "large_tr": (128, 128), "small_tr": (64, 64), "small32_tr": (32, 32)},
    "c128": {"large": (64, 16), "large_tr": (64, 128), "large_tr_full": (64, 128), "small_tr": (64, 64),
             "small32_tr": (32, 32)},
}
SHAPED = ("large", "large_tr", "large_tr_full", "small_tr", "medium_tr", "medium_tr_full", "small32_tr")


def subtile_items(dtype, ops, kind="local"):
    """the sub-tiles each tile_kernel launch of this list runs, from the executor's own work items:
    {variant: (op, f0, s0, tf, ts, whole)}, arrays with one entry per work item.  op = the item's
    record of the executor's ordered list (offsets in bytes, both VEC flags as the executor set
    them), (f0, s0) the sub-tile's origin in the op and (tf, ts) its extent as tile_kernel computes
    them; whole = the FULL instantiation of run_tile (a BF x BS sub-tile of an op with both VEC
    flags), every other one is guarded"""
    t = NAMES[int(dtype)]
    w = costa_amd.work_export(dtype, ops, kind)
    m = w.meta
    launched = variants(dtype, ops, kind)
    out = {}
    for lo, n, names in ((0, m["n_large"], ("large", "large_tr", "large_tr_full", "small_tr")),
                         (m["n_large"], m["n_medium"], ("medium_tr", "medium_tr_full", "small32_tr"))):
        if n <= 0:
            continue
        (v,) = [x for x in names if x in launched]
        bf, bs = _DIMS[t][v]
        item = w.work[lo:lo + n]
        op = w.ordered[(item >> np.uint64(32)).astype(np.int64)]
        sub = (item & np.uint64(0xFFFFFFFF)).astype(np.int64)
        nf, ns = op["nf"].astype(np.int64), op["ns"].astype(np.int64)
        nbf = (nf + bf - 1) // bf
        f0, s0 = sub % nbf * bf, sub // nbf * bs
        tf = np.minimum(bf, nf - f0)
        ts = np.minimum(bs, ns - s0)
        assert (tf > 0).all() and (ts > 0).all()
        both = (op["flags"] & (VEC_SRC | VEC_DST)) == (VEC_SRC | VEC_DST)
        whole = (tf == bf) & (ts == bs) & both
        out[v] = (op, f0, s0, tf, ts, whole)
    return out


def subtiles(dtype, ops, kind="local"):
    """the sub-tiles of subtile_items counted as tile_kernel sorts them:
    {variant: {"whole": n, "guarded": n, "whole_tr": n, "guarded_tr": n}}.  whole = the FULL
    instantiation of run_tile (a BF x BS sub-tile of an op with both VEC flags, as the executor's
    ordered list carries them), guarded = every other one; *_tr: those of transposing ops"""
    out = {}
    for v, (op, _, _, _, _, whole) in subtile_items(dtype, ops, kind).items():
        tr = (op["flags"] & TR) != 0
        out[v] = {"whole": int(whole.sum()), "guarded": int((~whole).sum()),
                  "whole_tr": int((whole & tr).sum()), "guarded_tr": int((~whole & tr).sum())}
    return out


def possible(t):
    """every name variants() can return for type t ("f32", ...), by the same rules"""
    alias = _ALIAS[t]
    out = {"large", alias.get("large_tr", "large_tr"), alias.get("large_tr_full", "large_tr_full"), "small32_tr"}
    if t in _HAS_SMALL:
        out.add("small_tr")
    if t in _HAS_MEDIUM:
        out |= {alias.get("medium_tr", "medium_tr"), alias.get("medium_tr_full", "medium_tr_full")}
    if t in REAL:
        out |= {"skew"} | ({"skew_wide"} if t in ("f32", "i32") else set())
        out |= {f"cblock_{s}{p}" for s in ("N", "T", "Nax", "Tax") for p in ("", "+pieces")}
    return out | {f"tiny_{s}" for s in ("N", "T", "Nax", "Tax")}


# ---------------------------------------------------------------------------- data
def _values(rng, dt, n):
    if dt == np.int32:
        return rng.integers(-1000, 1000, n, dtype=np.int32)
    x = rng.standard_normal(n)
    if np.issubdtype(dt, np.complexfloating):
        x = x + 1j * rng.standard_normal(n)
    return x.astype(dt)


def _data(rng, code, ops, n_src, n_dst):
    """-> (ops, source, initial destination, slot scalars), the data drawn in this order.
    SLOTS: 0 = (1, 0) bit copy / unit scale, 1 = (0, 0), 2 = (alpha, 0), 3 = (alpha, beta)"""
    dt = oracle.NP[code]
    src = _values(rng, dt, n_src)
    dst0 = _values(rng, dt, n_dst)
    if dt == np.int32:
        scal = np.array([1, 0, 0, 0, 2, 0, -3, 5], dt)
    else:
        a, b = _values(rng, dt, 2)
        scal = np.array([1, 0, 0, 0, a, 0, a, b], dt)
    return ops, src, dst0, scal


def _vec(E, src_off, lds, dst_off, ldd):
    f = 0
    if (src_off * E) % 16 == 0 and (lds * E) % 16 == 0:
        f |= VEC_SRC
    if (dst_off * E) % 16 == 0 and (ldd * E) % 16 == 0:
        f |= VEC_DST
    return f


def _scale(rng, tr, conj, kinds=4):
    """(kind, slot) agreeing with the slot scalars; kinds = 3: no beta*C op"""
    kind = int(rng.integers(0, kinds))
    if kind == 0 and (tr or conj):  # the planner never bit-copies through a transpose/conj
        return 2, 0                 # alpha = 1, beta = 0 evaluated as a product (memory_utils.hpp:101-291)
    return kind, ((0, 1, 2, 3)[kind] if kind != 2 else int(rng.choice([0, 2])))


# ---------------------------------------------------------------------------- the lists
def _shape(rng, E, transpose):
    """(nf, ns) drawn to hit every class and the boundaries between them"""
    pick = rng.integers(0, 8)
    if pick == 0:  # tiny, ragged
        return int(rng.integers(1, 70)), int(rng.integers(1, 70))
    if pick == 1:  # at the tiny boundary
        limit = (TINY_LDS if transpose else tiny_copy(E, bool(rng.integers(0, 2)))) // E
        nf = int(rng.integers(1, 129))
        ns = max(1, limit // ((nf | 1) if transpose else nf) + int(rng.integers(-1, 2)))
        return nf, ns
    if pick == 2:  # thin column
        return 1, int(rng.integers(1, 5000))
    if pick == 3:  # thin row
        return int(rng.integers(1, 5000)), 1
    if pick == 4:  # medium (small shape)
        return int(rng.integers(60, 200)), int(rng.integers(40, 140))
    if pick == 5:  # large shape, ragged edge
        return int(rng.integers(200, 600)), int(rng.integers(100, 300))
    if pick == 6:  # around the medium shape (256 threads, 16 KiB sub-tiles) of transposing lists
        return int(rng.integers(16, 100)), int(rng.integers(16, 100))
    return int(rng.integers(1, 400)), int(rng.integers(1, 400))


def _random_list(rng, code, n_ops, copy_only=False, kinds=4):
    """op list whose scale kinds agree with the slot scalars (see _data); copy_only: no
    transposing op (the executor then runs large ops on its copy shape); kinds = 3: no beta*C op"""
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    cplx = np.issubdtype(dt, np.complexfloating)
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        tr = bool(rng.integers(0, 2)) and not copy_only
        nf, ns = _shape(rng, E, tr)
        lds = nf + int(rng.integers(0, 2)) * int(rng.integers(0, 5))
        dn = ns if tr else nf
        ldd = dn + int(rng.integers(0, 2)) * int(rng.integers(0, 5))
        d_slow = nf if tr else ns
        if rng.integers(0, 3) == 0:  # misalign the start by a few elements
            src_off += int(rng.integers(1, 4))
            dst_off += int(rng.integers(1, 4))
        else:  # 16-byte aligned
            src_off = -(-src_off * E // 16) * 16 // E
            dst_off = -(-dst_off * E // 16) * 16 // E
        conj = bool(cplx and rng.integers(0, 2))
        kind, slot = _scale(rng, tr, conj, kinds)
        flags = (1 if tr else 0) | (2 if conj else 0) | (kind << 4) | (slot << 16)
        flags |= _vec(E, src_off, lds, dst_off, ldd)
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, flags, 0)
        src_off += (ns - 1) * lds + nf
        dst_off += (d_slow - 1) * ldd + dn
    return ops, src_off, dst_off


def mixed_list(code, seed):
    """240 random ops over every work class and the boundaries between them, every scale kind;
    seed "copy": no transposing op.  Shaped sub-tiles: whole and ragged-edge both (ops of 200-600 x
    100-300 and up to 400 x 400 on the large shapes)."""
    copy_only = seed == "copy"
    rng = np.random.default_rng(1000 * (7 if copy_only else seed) + code)
    ops, n_src, n_dst = _random_list(rng, code, 240, copy_only)
    return (rng, code, ops, n_src, n_dst)


def noax_list(code, copy_only):
    """the mixed recipe with scale kinds 0-2 only: no op reads its destination, so the wavefront
    and group kernels run their AX = false instantiations (tile_kernels.hip launch_tiny /
    launch_cblock) and the large shapes never load C.  Whole and ragged-edge sub-tiles both."""
    rng = np.random.default_rng(5100 + 10 * code + copy_only)
    ops, n_src, n_dst = _random_list(rng, code, 120, copy_only, kinds=3)
    return (rng, code, ops, n_src, n_dst)


def medium_list(code, nb, full):
    """a transposing list of 4200 aligned ops of about nb x nb (engine.cpp kMinMediumOps: the medium
    class only runs for lists of >= 4096 such ops), every scale kind and padded strides.  nb > 32:
    ops of nb or one 16-byte vector less along f.  4-byte types, 64 x 64 sub-tiles: nb = 64 whole
    and ragged-edge sub-tiles, nb = 80 ragged-edge ones only; fp64, 32 x 64 sub-tiles: nb = 48
    ragged-edge ones only (48 < 64: medium_mix_list has the whole ones); full: every op a whole medium sub-tile and no beta*C op (`medium_tr_full`, whole
    sub-tiles only by definition); nb == 32: 32 x 32 ops with 1 in 25 partly filled (`small32_tr`:
    whole and ragged-edge sub-tiles); nb < 32: every sub-tile would be partly filled, which build_work
    refuses (n_exact < 9/10): the negative case, all ops on the wavefront / group path"""
    rng = np.random.default_rng(77 + code + nb)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    n_ops = 4200
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        # full, or (above 32) one 16-byte vector short: every op stays in the medium class
        nf = nb - (int(rng.integers(0, 2)) * (16 // E) if nb > 32 and not full else 0)
        ns = nb
        if nb == 32 and rng.integers(0, 25) == 0:  # a few partly filled 32 x 32 sub-tiles
            nf, ns = int(rng.integers(17, 33)), int(rng.integers(17, 33))
        lds = nf + int(rng.integers(0, 2)) * (16 // E)
        ldd = ns + int(rng.integers(0, 2)) * (16 // E)
        kind = int(rng.integers(1, 3 if full else 4))  # full: no C read (the 128-thread launch)
        slot = (0, 1, 2, 3)[kind] if kind != 2 else int(rng.choice([0, 2]))
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, 1 | 4 | 8 | (kind << 4) | (slot << 16), 0)
        src_off += -(-((ns - 1) * lds + nf) * E // 16) * 16 // E
        dst_off += -(-((nf - 1) * ldd + ns) * E // 16) * 16 // E
    return (rng, code, ops, src_off, dst_off)


def medium_mix_list(code, ax):
    """a transposing list of 4200 aligned ops in the medium class of fp64 (32 x 64 sub-tiles): half
    of them exactly one sub-tile (the FULL path of run_tile), the rest short by 1-2 16-byte vectors
    along f, by 1-26 elements along s, or both (its guarded path), none above 32 x 64, so every
    sub-tile is whole or ragged-edge; padded strides; scale kinds 1-3, or 1-2 without ax (no op reads
    its destination).  `medium_tr` (fp64 `medium_tr_full` is the same kernel)"""
    rng = np.random.default_rng(7700 + 10 * code + ax)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    V = 16 // E
    bf, bs = _DIMS[NAMES[code]]["medium_tr"]
    n_ops = 4200
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        nf, ns = bf, bs
        if i % 2:
            cut = int(rng.integers(1, 4))
            if cut & 1:
                nf -= V * int(rng.integers(1, 3))
            if cut & 2:
                ns -= int(rng.integers(1, 27))
        assert 2 * nf * ns >= bf * bs
        lds = nf + int(rng.integers(0, 2)) * V
        ldd = -(-ns // V) * V + int(rng.integers(0, 2)) * V
        kind = int(rng.integers(1, 4 if ax else 3))
        slot = (0, 1, 2, 3)[kind] if kind != 2 else int(rng.choice([0, 2]))
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, 1 | 4 | 8 | (kind << 4) | (slot << 16), 0)
        src_off += -(-((ns - 1) * lds + nf) * E // 16) * 16 // E
        dst_off += -(-((nf - 1) * ldd + ns) * E // 16) * 16 // E
    return (rng, code, ops, src_off, dst_off)


def whole_tr_list(code):
    """24 aligned transposing ops for the large transposing shape of 4-byte types (128 x 128): two
    in three whole multiples of it up to 384 x 256 (the FULL path of run_tile on transposing ops),
    the rest 130-400 x 130-300 (ragged-edge sub-tiles), every scale kind; destination leading
    dimensions padded to multiples of 64 bytes (off that granule a transposing op goes to the skew
    rule and out of the large class)"""
    rng = np.random.default_rng(8800 + code)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    G = 64 // E
    bf, bs = _DIMS[NAMES[code]]["large_tr"]
    n_ops = 24
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        if i % 3 != 2:
            nf, ns = bf * int(rng.integers(1, 4)), bs * int(rng.integers(1, 3))
        else:
            nf, ns = int(rng.integers(130, 401)), int(rng.integers(130, 301))
        lds = -(-nf // G) * G + G * int(rng.integers(0, 2))
        ldd = -(-ns // G) * G + G * int(rng.integers(0, 2))
        kind, slot = _scale(rng, True, False)
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, 1 | _vec(E, src_off, lds, dst_off, ldd) | (kind << 4) | (slot << 16), 0)
        src_off += -(-((ns - 1) * lds + nf) // G) * G
        dst_off += -(-((nf - 1) * ldd + ns) // G) * G
    return (rng, code, ops, src_off, dst_off)


def unaligned_list(code, copy_only):
    """40 large ops (100-420 x 100-300) whose columns are not 16-byte aligned on one side or both
    (odd lld for 8-byte types, lld % 4 != 0 for 4-byte ones): the large shape's element-wise path
    (tile_kernels.hip run_tile_elem), whole and ragged-edge sub-tiles, every scale kind"""
    rng = np.random.default_rng(4242 + code + 10 * copy_only)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    cplx = np.issubdtype(dt, np.complexfloating)
    n_ops = 40
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        tr = bool(rng.integers(0, 2)) and not copy_only
        nf, ns = int(rng.integers(100, 420)), int(rng.integers(100, 300))
        side = int(rng.integers(0, 3))  # 0: source unaligned, 1: destination, 2: both
        lds = nf + (int(rng.integers(0, 3)) * 2 + 1 if side != 1 else 16 // E)
        dn, d_slow = (ns, nf) if tr else (nf, ns)
        ldd = dn + (int(rng.integers(0, 3)) * 2 + 1 if side != 0 else 16 // E)
        src_off = -(-src_off * E // 16) * 16 // E + (int(rng.integers(0, 2)) if side != 1 else 0)
        dst_off = -(-dst_off * E // 16) * 16 // E + (int(rng.integers(0, 2)) if side != 0 else 0)
        conj = bool(cplx and rng.integers(0, 2))
        kind, slot = _scale(rng, tr, conj)
        flags = (1 if tr else 0) | (2 if conj else 0) | (kind << 4) | (slot << 16)
        flags |= _vec(E, src_off, lds, dst_off, ldd)
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, flags, 0)
        src_off += (ns - 1) * lds + nf
        dst_off += (d_slow - 1) * ldd + dn
    return (rng, code, ops, src_off, dst_off)


def square_list(code, seed):
    """600 ops, 3 in 4 transposing, whose large ops all fit 64 x 64 (nb = 64 blocks): they run on the
    square variant of the transposing shape (engine.cpp build_work sq, tile_kernels.hip small_tr).
    8 in 15 ops fill a sub-tile exactly, 4 in 15 are 46-64 a side, the rest are small ops for the
    wavefront path.  c64 / c128 (no medium tier: the large class starts at half a square sub-tile):
    whole and ragged-edge sub-tiles.  fp64: whole sub-tiles only, and no list can do better: with the
    square shape on, the large class starts at q_lo = sub_elems = 64 x 128 / 2 elements, so an op must
    hold 4096 elements and fit 64 x 64, i.e. be exactly 64 x 64, and an unaligned one goes to the
    wavefront path (wave policy 2, kUnalignedWaveCap); the 46-64 ops run there too; padded and unaligned strides, every scale kind (conjugation
    for complex types)"""
    rng = np.random.default_rng(640 + seed + 10 * code)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    cplx = np.issubdtype(dt, np.complexfloating)
    n_ops = 600
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        tr = rng.integers(0, 4) != 0
        nf, ns = ((64, 64) if rng.integers(0, 3) else (int(rng.integers(46, 65)), int(rng.integers(46, 65)))) \
            if rng.integers(0, 5) else (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        lds = nf + int(rng.integers(0, 3)) * int(rng.integers(0, 2))
        dn, d_slow = (ns, nf) if tr else (nf, ns)
        ldd = dn + int(rng.integers(0, 3)) * int(rng.integers(0, 2))
        if rng.integers(0, 4) == 0:
            src_off += 1
            dst_off += 1
        else:
            src_off = -(-src_off * E // 16) * 16 // E
            dst_off = -(-dst_off * E // 16) * 16 // E
        conj = bool(cplx and rng.integers(0, 2))
        kind, slot = _scale(rng, tr, conj)
        flags = (1 if tr else 0) | (2 if conj else 0) | (kind << 4) | (slot << 16)
        flags |= _vec(E, src_off, lds, dst_off, ldd)
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, flags, 0)
        src_off += (ns - 1) * lds + nf
        dst_off += (d_slow - 1) * ldd + dn
    return (rng, code, ops, src_off, dst_off)


def full_list(code, kinds=4, extra=False):
    """40 aligned ops, 3 in 4 transposing, each a whole multiple of the large transposing sub-tile
    (c128 and fp64: 64 x 128) up to 192 x 256, leading dimensions equal to the extent or padded by
    64 bytes (a destination column off the 64-byte granule would send an fp64 op to the skew rule and
    out of the large class), every scale kind below `kinds` (conjugation for c128).  Every sub-tile
    is whole: engine.cpp work_split::full.
    extra (c128): one ragged transposing op (128 x 20 or 20 x 128) that is a candidate of the square
    shape but fits no 64 x 64 sub-tile, which switches the square shape off (without it a c128 list
    of aligned multiples of 64 x 64 takes `small_tr` first), and 12 small ops for the wavefront path,
    so the shaped and the tiny launch both run in one call"""
    rng = np.random.default_rng(9100 + code + 100 * (4 - kinds))
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    cplx = np.issubdtype(dt, np.complexfloating)
    n_ops = 40 + (13 if extra else 0)
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        tr = i == 0 or rng.integers(0, 4) != 0
        nf, ns = 64 * int(rng.integers(1, 4)), 128 * int(rng.integers(1, 3))
        if i == 40:  # the ragged candidate of the square shape
            tr, (nf, ns) = True, ((128, 20), (20, 128))[int(rng.integers(0, 2))]
        elif i > 40:
            nf, ns = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        lds = nf + (64 // E) * int(rng.integers(0, 2))
        dn, d_slow = (ns, nf) if tr else (nf, ns)
        ldd = dn + (64 // E) * int(rng.integers(0, 2))
        conj = bool(cplx and rng.integers(0, 2))
        kind, slot = _scale(rng, tr, conj, kinds)
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd,
                  (1 if tr else 0) | (2 if conj else 0) | _vec(E, src_off, lds, dst_off, ldd) | (kind << 4) | (slot << 16), 0)
        src_off += -(-((ns - 1) * lds + nf) * E // 64) * 64 // E
        dst_off += -(-((d_slow - 1) * ldd + dn) * E // 64) * 64 // E
    return (rng, code, ops, src_off, dst_off)


def phase_list(code, seed):
    """600 wavefront transposes of 4-byte elements into destination columns at every 16-byte phase:
    every destination offset mod 4, leading dimensions ns .. ns + 3 (each column starting at another
    phase), heights 1 .. 160, widths 1 .. 64, ops the host cuts into pieces, scale kinds 1-3;
    neighbouring ops' destination columns share 16-byte chunks; 8 guard elements after the last op"""
    rng = np.random.default_rng(9300 + 10 * seed + code)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    n_ops = 600
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        nf = int(rng.integers(1, 65))
        ns = int(rng.choice([int(rng.integers(1, 12)), int(rng.integers(8, 161))]))
        lds = nf + int(rng.integers(0, 4))
        ldd = ns + int(rng.integers(0, 4))
        src_off += int(rng.integers(0, 4))
        dst_off += int(rng.integers(0, 4))
        kind = int(rng.integers(1, 4))
        slot = (0, 1, 2, 3)[kind] if kind != 2 else int(rng.choice([0, 2]))
        flags = 1 | (kind << 4) | (slot << 16) | _vec(E, src_off, lds, dst_off, ldd)
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, flags, 0)
        src_off += (ns - 1) * lds + nf
        # the next op's destination starts inside this op's last column's padding (ldd > ns) or
        # right after it: 16-byte chunks are shared between ops
        dst_off += (nf - 1) * ldd + ns
    return (rng, code, ops, src_off, dst_off + 8)


def wave_list(code, tr):
    """200 small ops (1-48 x 1-40) for the wavefront path alone, scale kinds 0-2 (no op reads its
    destination: tile_kernels.hip tiny_kernel<T, *, tr, AX = false>), padded strides, every
    alignment; tr: half the ops transpose (conjugation for complex types).  1-3 elements that no op
    may write lie between neighbouring ops' destinations, so no two ops form a destination-block
    group; 8 guard elements after the last op"""
    rng = np.random.default_rng(6200 + 10 * code + tr)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    cplx = np.issubdtype(dt, np.complexfloating)
    n_ops = 200
    ops = np.zeros(n_ops, costa_amd.TILE_OP_DTYPE)
    src_off = dst_off = 0
    for i in range(n_ops):
        t = bool(tr and (i == 0 or rng.integers(0, 2)))
        nf, ns = int(rng.integers(1, 49)), int(rng.integers(1, 41))  # (c128: below half a 64 x 64 sub-tile)
        lds = nf + int(rng.integers(0, 4))
        dn, d_slow = (ns, nf) if t else (nf, ns)
        ldd = dn + int(rng.integers(0, 4))
        src_off += int(rng.integers(0, 4))
        dst_off += int(rng.integers(1, 4))
        conj = bool(cplx and rng.integers(0, 2))
        kind, slot = _scale(rng, t, conj, 3)
        flags = (1 if t else 0) | (2 if conj else 0) | (kind << 4) | (slot << 16) | _vec(E, src_off, lds, dst_off, ldd)
        ops[i] = (src_off * E, dst_off * E, nf, ns, lds, ldd, flags, 0)
        src_off += (ns - 1) * lds + nf
        dst_off += (d_slow - 1) * ldd + dn
    return (rng, code, ops, src_off, dst_off + 8)


def _guillotine(rng, r0, r1, c0, c1, max_area, out):
    """random guillotine cuts of [r0, r1) x [c0, c1) into rectangles of at most max_area"""
    h, w = r1 - r0, c1 - c0
    if h * w <= max_area or (h == 1 and w == 1):
        out.append((r0, r1, c0, c1))
        return
    if (w >= h or h == 1) and w > 1:
        c = int(rng.integers(c0 + 1, c1))
        _guillotine(rng, r0, r1, c0, c, max_area, out)
        _guillotine(rng, r0, r1, c, c1, max_area, out)
    else:
        r = int(rng.integers(r0 + 1, r1))
        _guillotine(rng, r0, r, c0, c1, max_area, out)
        _guillotine(rng, r, r1, c0, c1, max_area, out)


def group_list(code, tr, ax, pieces):
    """28 destination blocks, ragged, 8-160 a side (BASELINE cfg 5's range), each a column-major
    buffer of its own leading dimension tiled exactly by 2 or more ops that read separate sources:
    engine.cpp cblock_groups makes each a destination-block group (blocks above the workgroup's budget
    several, cut in column bands), run by tile_kernels.hip cblock_kernel<T, tr, ax>.  One transform a
    block; tr: 3 in 4 blocks transpose (the rest copy, in the same launch); ax: scale kinds 0-3, else
    0-2 (no op reads its destination); 1-5 elements between blocks that no op may write, 8 after the
    last.  pieces: 10 more ops, each alone in its buffer, stay on the wavefront path and ride in the
    group launch's tail (launch_t: pieces_in_group_launch); without them every op is grouped and no
    wavefront launch runs."""
    rng = np.random.default_rng(7000 + 100 * code + 4 * tr + 2 * ax + pieces)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    rows = []
    src_off = dst_off = 0
    for b in range(28 + (10 if pieces else 0)):
        lone = b >= 28
        R, K = (int(rng.integers(1, 40)), int(rng.integers(1, 40))) if lone else \
            (int(rng.integers(8, 161)), int(rng.integers(8, 161)))
        t = bool(tr and rng.integers(0, 4) != 0)
        kind, slot = _scale(rng, t, False, 4 if ax else 3)
        if ax and b == 0:
            kind, slot = 3, 3
        rects = []
        if lone:
            rects.append((0, R, 0, K))
        else:
            while len(rects) < 2:
                rects.clear()
                _guillotine(rng, 0, R, 0, K, min(int(rng.choice([64, 300, 2000])), R * K // 2), rects)
        for r0, r1, c0, c1 in rects:
            run, runs = r1 - r0, c1 - c0
            nf, ns = (runs, run) if t else (run, runs)
            lds = nf + int(rng.integers(0, 3))
            d = dst_off + c0 * R + r0
            flags = (1 if t else 0) | (kind << 4) | (slot << 16) | _vec(E, src_off, lds, d, R)
            rows.append((src_off * E, d * E, nf, ns, lds, R, flags, 0))
            src_off += (ns - 1) * lds + nf + int(rng.integers(0, 3))
        dst_off += R * K + int(rng.integers(1, 6))
    ops = np.array(rows, costa_amd.TILE_OP_DTYPE)
    ops = ops[rng.permutation(ops.size)]  # list order != destination order
    return (rng, code, ops, src_off, dst_off + 8)


def skew_list(code, on16, wide):
    """One transposing matrix cut into a 3 x 4 grid of ops whose destination leading dimension is
    above the group budget (engine.cpp build_work: below it such ops stay on the wavefront path) and
    off the 16-byte grid (on16 = False) or on it but off the 64-byte one (on16 = True): every op holds
    more than half a skew sub-tile (4-byte types 32 x 512, wide 64 x 256; fp64 64 x 128) and goes to
    tile_kernels.hip skew_kernel.  Widths and heights are no multiples of the sub-tile (whole and
    ragged-edge sub-tiles both); ops stacked in a destination column share the granule at their
    common edge; one scale kind (1-3) per op, except that the two lower ops of the first panel and the
    whole third column of ops share theirs and continue each other in source and destination, so
    merge_adjacent joins them (along s and along f: at most 10 of the 12 ops are left, fewer when
    neighbours draw the same kind).  wide (4-byte types): the source panels start off the 16-byte grid
    and the source leading dimension is odd (`skew_wide`); else 4-byte sources are 16-byte aligned,
    while two of the three fp64 source panels start 8 bytes off the grid (element loads there).  The destination starts a few elements into its buffer; 8 guard elements after."""
    rng = np.random.default_rng(8300 + 10 * code + 2 * on16 + wide)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    V = 16 // E
    G = 64 // E
    ldd = -(-group_budget(E) // G) * G + (V if on16 else V + 1)
    assert ldd > group_budget(E) and (ldd * E % 16 == 0) == on16 and ldd * E % 64 != 0
    fcut = [0, 37, 101, 150] if wide or E == 8 else [0, 36, 100, 152]
    top = ldd - 3
    scut = [0, top // 6 + 1, top // 6 + 1 + 4096 // E // 8 * 3, top // 2 + 5, top]
    lds = fcut[-1] + (1 if wide else V)
    d0 = V if on16 else 3
    shared = AXPBY  # the merged ops read C
    rows = []
    for i in range(3):
        for j in range(4):
            f0, f1, s0, s1 = fcut[i], fcut[i + 1], scut[j], scut[j + 1]
            kind = shared if (i == 0 and j >= 2) or j == 2 else int(rng.integers(1, 4))
            slot = (0, 1, 2, 3)[kind] if kind != 2 else (2 if (i == 0 and j >= 2) or j == 2 else int(rng.choice([0, 2])))
            s_at, d_at = s0 * lds + f0, d0 + f0 * ldd + s0
            flags = 1 | (kind << 4) | (slot << 16) | _vec(E, s_at, lds, d_at, ldd)
            rows.append((s_at * E, d_at * E, f1 - f0, s1 - s0, lds, ldd, flags, 0))
    ops = np.array(rows, costa_amd.TILE_OP_DTYPE)
    assert (2 * ops["nf"].astype(np.int64) * ops["ns"] >= (16384 if E == 4 else 8192)).all()
    ops = ops[rng.permutation(ops.size)]
    return (rng, code, ops, (scut[-1] - 1) * lds + fcut[-1], d0 + (fcut[-1] - 1) * ldd + scut[-1] + 8)


# ---------------------------------------------------------------------------- the registry
# name -> (dtype code, builder, the launches the list exists to exercise)
LISTS = {}
# name -> {meta field: value} the split must show besides (tests assert them with the route)
SPLIT = {}


def _add(name, t, builder, declared, **split_expect):
    assert name not in LISTS
    LISTS[name] = (CODES[t], builder, frozenset(declared))
    if split_expect:
        SPLIT[name] = split_expect


def _p(fn, *a, **k):
    return functools.partial(fn, *a, **k)


def _register():
    cx = lambda t, s: {f"tiny_{s}"} if t in ("c64", "c128") else set()  # noqa: E731
    # every class at once (real types: their wavefront pieces may ride in a group launch, which the
    # group lists pin; undeclared here)
    for seed in (1, 2, 3):
        for t, c in CODES.items():
            _add(f"mixed[{seed}-{t}]", t, _p(mixed_list, c, seed), {"large_tr"} | cx(t, "Tax"))
    for t, c in CODES.items():
        _add(f"mixed[copy-{t}]", t, _p(mixed_list, c, "copy"), {"large"} | cx(t, "Nax"))
    # the medium class
    _add("medium[f32-64]", "f32", _p(medium_list, 0, 64, False), {"medium_tr"}, n_large=0)
    _add("medium[f64-32]", "f64", _p(medium_list, 1, 32, False), {"small32_tr"}, n_large=0)
    _add("medium[f64-48]", "f64", _p(medium_list, 1, 48, False), {"medium_tr"}, n_large=0)
    _add("medium[f64-mix]", "f64", _p(medium_mix_list, 1, True), {"medium_tr"}, n_large=0, med_full=False)
    _add("medium[f64-mix-noax]", "f64", _p(medium_mix_list, 1, False), {"medium_tr"}, n_large=0, med_full=False)
    _add("medium[i32-64]", "i32", _p(medium_list, 4, 64, False), {"medium_tr"}, n_large=0)
    _add("medium[f32-80]", "f32", _p(medium_list, 0, 80, False), {"medium_tr"}, n_large=0)
    _add("medium[f32-64-full]", "f32", _p(medium_list, 0, 64, True), {"medium_tr_full"}, n_large=0)
    _add("medium[i32-64-full]", "i32", _p(medium_list, 4, 64, True), {"medium_tr_full"}, n_large=0)
    _add("medium[f32-32]", "f32", _p(medium_list, 0, 32, False), {"small32_tr"}, n_large=0)
    _add("medium[c64-32]", "c64", _p(medium_list, 2, 32, False), {"small32_tr"}, n_large=0)
    _add("medium[c128-32]", "c128", _p(medium_list, 3, 32, False), {"small32_tr"}, n_large=0)
    _add("medium[i32-32]", "i32", _p(medium_list, 4, 32, False), {"small32_tr"}, n_large=0)
    # the negative case: 24 x 24 ops only part-fill 32 x 32 sub-tiles, so no medium launch at all
    _add("medium[i32-24]", "i32", _p(medium_list, 4, 24, False), {"cblock_Tax+pieces"}, n_medium=0, n_large=0)
    for t, c in CODES.items():
        _add(f"unaligned[mixed-{t}]", t, _p(unaligned_list, c, False), {"large_tr", "tiny_Tax"})
        _add(f"unaligned[copy-{t}]", t, _p(unaligned_list, c, True), {"large", "tiny_Nax"})
    for seed in (1, 2):
        for t in ("f64", "c64", "c128"):
            _add(f"square[{seed}-{t}]", t, _p(square_list, CODES[t], seed), {"small_tr"}, sq=True)
    # all-whole large sub-tiles: c128's own 256-thread kernel; fp64's `full` launch is large_tr itself
    _add("full[c128]", "c128", _p(full_list, 3, 4, True), {"large_tr_full", "tiny_Tax"}, full=True, sq=False)
    _add("full[c128-noax]", "c128", _p(full_list, 3, 3, True), {"large_tr_full", "tiny_T"}, full=True, sq=False)
    _add("full[f64]", "f64", _p(full_list, 1), {"large_tr"}, full=True, sq=False, n_tiny=0, n_skew=0)
    # 4-byte types: whole sub-tiles of transposing ops on large_tr, which the random lists only draw by luck
    for t in ("f32", "i32"):
        _add(f"full[{t}-mix]", t, _p(whole_tr_list, CODES[t]), {"large_tr"}, full=False, n_skew=0, n_medium=0)
    for seed in (1, 2):
        for t in ("f32", "i32"):
            _add(f"phase[{seed}-{t}]", t, _p(phase_list, CODES[t], seed), {"tiny_Tax"}, n_cblock=0)
    # no beta*C op anywhere
    for t, c in CODES.items():
        _add(f"noax[copy-{t}]", t, _p(noax_list, c, True), {"large"} | cx(t, "N"))
        _add(f"noax[mixed-{t}]", t, _p(noax_list, c, False), {"large_tr"} | cx(t, "T"))
        _add(f"wave[N-{t}]", t, _p(wave_list, c, False), {"tiny_N"}, n_large=0, n_cblock=0)
        _add(f"wave[T-{t}]", t, _p(wave_list, c, True), {"tiny_T"}, n_large=0, n_cblock=0)
    # destination-block groups, every instantiation of cblock_kernel, with and without pieces
    for t in REAL:
        for tr in (False, True):
            for ax in (False, True):
                for pieces in (False, True):
                    s = ("T" if tr else "N") + ("ax" if ax else "")
                    _add(f"group[{s}{'+p' if pieces else ''}-{t}]", t, _p(group_list, CODES[t], tr, ax, pieces),
                         {f"cblock_{s}" + ("+pieces" if pieces else "")}, n_large=0, n_medium=0, n_skew=0)
    # the skew shape
    for t in REAL:
        _add(f"skew[off16-{t}]", t, _p(skew_list, CODES[t], False, False), {"skew"}, n_large=0, n_tiny=0, n_ordered_max=10)
        _add(f"skew[off64-{t}]", t, _p(skew_list, CODES[t], True, False), {"skew"}, n_large=0, n_tiny=0, n_ordered_max=10)
    for t in ("f32", "i32"):
        _add(f"skew[wide-off16-{t}]", t, _p(skew_list, CODES[t], False, True), {"skew_wide"}, n_large=0, n_tiny=0, n_ordered_max=10)
        _add(f"skew[wide-off64-{t}]", t, _p(skew_list, CODES[t], True, True), {"skew_wide"}, n_large=0, n_tiny=0, n_ordered_max=10)


_register()


def ops_of(name):
    """-> (dtype code, ops) of a registry list"""
    code, builder, _ = LISTS[name]
    return code, builder()[2]


def extents(name):
    """-> (dtype code, ops, n_src, n_dst): the element counts of the two buffers"""
    _, code, ops, n_src, n_dst = LISTS[name][1]()
    return code, ops, n_src, n_dst


# oracle.add_specials seeds of the source and of the initial destination in the special-value modes
SPECIAL_SEEDS = (0x5A11, 0x5C22)


def build(name, specials=None):
    """-> (dtype code, ops, src, dst0, scalars, declared) of a registry list.  specials = "drawn":
    oracle.add_specials (about one element in 8 with parts from {+-inf, NaN, +-0, huge, -3, 0.5}, the
    golden specials' rule) over the drawn source and initial destination, the drawn scalars kept;
    "huge": slots 2 and 3 take specials_common.HUGE's pair besides (alpha * x overflows: Annex G's recovery with
    no infinite input)"""
    assert specials in (None, "drawn", "huge"), specials
    code, builder, declared = LISTS[name]
    ops, src, dst0, scal = _data(*builder())
    if specials is not None:
        assert NAMES[code] != "i32", "add_specials leaves integers as they are"
        src = oracle.add_specials(src, code, SPECIAL_SEEDS[0], 0)
        dst0 = oracle.add_specials(dst0, code, SPECIAL_SEEDS[1], 0)
        if specials == "huge":
            a, b = specials_common.HUGE[np.dtype(oracle.NP[code])]
            scal = scal.copy()
            scal[4:8] = (a, 0, a, b)
    return code, ops, src, dst0, scal, declared


def expected(code, ops, scal, src, dst0):
    """the oracle's destination after the list, each op as the kind it carries
    (specials_common.exec_ops: the lists draw ALPHA with alpha = 1 on copy ops too, which the oracle's
    own rule would memcpy), and the mask of the elements its ops write"""
    exp = dst0.copy()
    specials_common.exec_ops(code, ops, scal, src.ctypes.data, exp.ctypes.data)
    return exp, specials_common.written(ops, dst0.size, dst0.itemsize)


def special_cells(name, specials):
    """-> (specials_common.redo_cells of the shaped launches the list declares, share of NaN parts
    among the expected real parts it writes): host and oracle only"""
    code, ops, src, dst0, scal, declared = build(name, specials)
    exp, mask = expected(code, ops, scal, src, dst0)
    share = specials_common.assert_nan_share(exp, mask, f"{name} {specials}")
    subs = (specials_common.Sub(v, op[i], int(f0[i]), int(s0[i]), int(tf[i]), int(ts[i]), bool(whole[i]))
            for v, (op, f0, s0, tf, ts, whole) in subtile_items(code, ops).items() if v in declared
            for i in range(f0.size))
    return specials_common.redo_cells(subs, src, dst0, exp, scal, 16 // dst0.itemsize), share


def check_route(name, ops=None):
    """declared <= variants(), and the split fields the list pins; host only -> (variants, split)"""
    code, _, declared = LISTS[name]
    if ops is None:
        ops = ops_of(name)[1]
    got = variants(code, ops)
    assert declared <= got, f"{name}: declared {sorted(declared)} but launch_t would issue {sorted(got)}"
    m = split(code, ops)
    for k, want in SPLIT.get(name, {}).items():
        if k.endswith("_max"):  # (skew lists: n_ordered = the ops left after merge_adjacent)
            assert m[k[:-4]] <= want, f"{name}: split has {k[:-4]} = {m[k[:-4]]}, the list needs at most {want}"
            continue
        assert m[k] == want, f"{name}: split has {k} = {m[k]}, the list needs {want} ({m})"
    return got, m
