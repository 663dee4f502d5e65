"""Stretched twins of the families' test cases: the same small matrices inside buffers whose
leading dimension (block-cyclic) or block placement (custom) puts part of them past 2^32 bytes or
2^31 elements (tests/test_gpu_extents.py, tests/test_extents_plan_cpu.py).

The *twin* is the ordinary small case; every expected value is computed on it by the family's own
CPU reference.  The *stretched* case has the same matrix, blocks and alignment class (its leading
dimension grows by a multiple of 256 elements, which keeps ld * E mod 64 bytes for every element
size down to the packed 4- and 6-bit types), so both sides keep their VEC flags and the kernels
take the same paths: only the address arithmetic sees larger numbers.  The stretched size exists on
the device alone: `upload` fills it with a sentinel byte there and copies the twin's data in through
a strided view; `check` compares the touched rectangle with the expected twin bit for bit, puts the
sentinel back and then asserts that EVERY other byte of the buffer still holds it, so a write whose
offset wrapped modulo 2^32 is found wherever it landed.  `buf_elems` of a stretched case raises: no
stretched size may reach numpy.

Before any launch the tests call `check_footprints` (every op inside its allocation; nothing is
launched when that fails) and `crossing` (the threshold is really crossed, inside one op, by the
sub-tiles of the lists that will run), both in Python integers on plan_export / work_export output.
"""
import dataclasses

import numpy as np

from casegen import BC, Custom

SENTINEL = 0xA5
BYTE_RULE = 1 << 32   # bytes between a sub-tile's first element and its op's first element
ELEM_RULE = 1 << 31   # ... in elements (element types of <= 4 bytes)
GIB = 1 << 30
SIDE_LIMIT = 12 * GIB  # one stretched side
TEST_LIMIT = 20 * GIB  # everything one test holds on the device
STEP = 256            # elements: ld * E mod 64 bytes is kept for E = 16 bytes .. 4 bits

# quarter-bytes per element of every element code (costa_hip.h): FP4 packs 2 per byte, FP6 4 per 3
QB = {0: 16, 1: 32, 2: 32, 3: 64, 4: 16, 5: 8, 6: 8, 7: 4, 8: 4, 9: 2, 10: 3, 11: 3}


def nbytes(code, n):
    """bytes of n elements of `code` (n a multiple of the packing group for the packed types)"""
    assert (n * QB[code]) % 4 == 0, (code, n)
    return n * QB[code] // 4


def threshold_elems(rule, code):
    """the rule's threshold in elements of `code`"""
    if rule == "bytes":
        return -(-BYTE_RULE * 4 // QB[code])
    assert rule == "elems" and QB[code] <= 16, (rule, code)
    return ELEM_RULE


# ------------------------------------------------------------------ stretched cases
@dataclasses.dataclass
class StretchedBC(BC):
    """a BC case whose lld is far larger than its local rows: device-only"""

    def buf_elems(self, rank, P):
        raise AssertionError("the size of a stretched case must never reach the host")

    def big_elems(self, P=1):
        return BC.sizes(self, P)[1]


def stretched(case, threshold, side=None, frac=0.75):
    """`case` (a BC) with lld_pad raised by a multiple of 256 elements so that local column (row,
    for row-major storage) ceil(frac * columns) starts `threshold` elements or more after the first:
    an op over the whole local matrix then has sub-tiles on both sides of the threshold.  `side`
    ("src" / "dst") only labels the copy."""
    assert isinstance(case, BC) and not isinstance(case, StretchedBC)
    lld, total = case.sizes(1)
    slow = total // lld
    j = max(1, int(np.ceil(frac * slow)))
    assert j < slow, f"{slow} local columns: none left past the threshold"
    want = -(-threshold // j)
    k = max(1, -(-(want - lld) // STEP))
    big = StretchedBC(**{f.name: getattr(case, f.name) for f in dataclasses.fields(BC)})
    big.lld_pad = case.lld_pad + k * STEP
    big.side = side
    new_lld = big.sizes(1)[0]
    assert new_lld == lld + k * STEP and j * new_lld >= threshold and new_lld < 2 ** 31
    return big


def with_lld(case, lld):
    """`case` (a BC) stretched to the first leading dimension >= lld that keeps its alignment class"""
    old = case.sizes(1)[0]
    big = StretchedBC(**{f.name: getattr(case, f.name) for f in dataclasses.fields(BC)})
    big.lld_pad = case.lld_pad + max(1, -(-(lld - old) // STEP)) * STEP
    assert big.sizes(1)[0] < 2 ** 31
    return big


class TwoArena:
    """a Custom case (one rank) whose blocks alternate between two arenas of ONE allocation, the
    second arena starting `gap` elements (a multiple of 256) after the first.  Every block keeps its
    leading dimension and its offset modulo 256 elements, so alignment and VEC flags are the twin's."""

    def __init__(self, case, gap):
        assert isinstance(case, Custom) and case.nranks == 1 and gap % STEP == 0
        self.twin, self.gap, self.ord = case, gap, case.ord
        per, _ = case._blocks(1)
        at = [0, gap]
        self.blocks = []  # (block row, block column, twin offset, big offset, ld, elements)
        for k, (i, j, off, ld) in enumerate(per[0]):
            rows = case.rowsplit[i + 1] - case.rowsplit[i]
            cols = case.colsplit[j + 1] - case.colsplit[j]
            fast, slow = (rows, cols) if case.ord == "C" else (cols, rows)
            n = ld * (slow - 1) + fast if slow > 0 and fast > 0 else 0
            a = k % 2
            pos = at[a] + (off - at[a]) % STEP
            self.blocks.append((i, j, off, pos, ld, n))
            at[a] = pos + n + case.gap
        assert at[0] <= gap, "the first arena runs into the second"
        self.elems = at[1] + STEP

    def buf_elems(self, rank, P):
        raise AssertionError("the size of a stretched case must never reach the host")

    def big_elems(self, P=1):
        return self.elems

    def shape(self):
        return self.twin.shape()


def make_layout(costa, case, ptr, code):
    """the product's one-rank layout of a twin or a stretched case over a buffer of `code` at `ptr`"""
    if isinstance(case, BC):
        return case.make_layout(0, ptr, 1, code)
    if isinstance(case, TwoArena):
        c = case.twin
        blocks = [(ptr + nbytes(code, big), ld, i, j) for i, j, _, big, ld, _ in case.blocks]
    else:
        c = case
        blocks = [(ptr + nbytes(code, off), ld, i, j) for i, j, off, ld in case._blocks(1)[0][0]]
    nbr, nbc = c.owners.shape
    return costa.custom_layout(nbr, nbc, c.rowsplit, c.colsplit, c.owners, blocks, c.ord, code)


def big_bytes(case, code):
    """bytes of the buffer of a stretched case (or of a twin, for a side that is not stretched)"""
    n = case.big_elems(1) if hasattr(case, "big_elems") else case.buf_elems(0, 1)
    return nbytes(code, n)


# ------------------------------------------------------------------ device buffers
def _rect(t, twin, big, code):
    """the strided view of device byte tensor `t` (the stretched buffer) that holds the twin's
    whole buffer: one row per local column, the twin's padding rows included"""
    lld_t, total = twin.sizes(1)
    slow = total // lld_t
    return t.as_strided((slow, nbytes(code, lld_t)), (nbytes(code, big.sizes(1)[0]), 1))


def _index(big, code):
    """twin byte -> stretched byte of every block of a TwoArena, as one device index tensor"""
    import torch
    src, dst = [], []
    for _, _, off, pos, _, n in big.blocks:
        src.append(np.arange(nbytes(code, off), nbytes(code, off + n), dtype=np.int64))
        dst.append(np.arange(nbytes(code, pos), nbytes(code, pos + n), dtype=np.int64))
    return (torch.from_numpy(np.concatenate(src)).cuda(), torch.from_numpy(np.concatenate(dst)).cuda())


def _dev_bytes(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def need(n_bytes):
    """skip only when the device reports less free memory than the test holds"""
    import pytest
    import torch
    assert n_bytes <= TEST_LIMIT, f"{n_bytes / GIB:.1f} GiB: a test holds at most 20 GiB"
    free = torch.cuda.mem_get_info()[0]
    if free < n_bytes + GIB:
        pytest.skip(f"{free / GIB:.1f} GiB free on the device, the test holds {n_bytes / GIB:.1f} GiB")


def upload(twin_buf, twin, big, code, sentinel=SENTINEL):
    """a device byte tensor of the stretched size: the sentinel everywhere, the twin's local data
    where the stretched layout has it.  (A block of a custom twin is copied without the gap after
    it; the bytes between a block's columns travel with it.)"""
    import torch
    size = big_bytes(big, code)
    assert size <= SIDE_LIMIT, f"{size / GIB:.1f} GiB: a stretched side stays below 12 GiB"
    t = torch.full((size,), sentinel, dtype=torch.uint8, device="cuda")
    small = _dev_bytes(twin_buf)
    if isinstance(big, BC):
        r = _rect(t, twin, big, code)
        assert small.numel() == r.shape[0] * r.shape[1]
        r.copy_(small.view(r.shape))
    else:
        src, dst = _index(big, code)
        t[dst] = small[src]
    return t


def assert_sentinel(t, what, sentinel=SENTINEL):
    """every byte of device tensor `t` equals the sentinel; chunks of 1 GiB"""
    import torch
    word = int.from_bytes(bytes([sentinel]) * 8, "little", signed=True)
    n8 = t.numel() // 8 * 8
    assert t.data_ptr() % 8 == 0
    w = t[:n8].view(torch.int64)
    step = GIB // 8
    for lo in range(0, w.numel(), step):
        ch = w[lo:lo + step]
        ok = bool((ch == word).all())
        if not ok:
            at = 8 * (lo + int(torch.nonzero(ch != word)[0, 0]))
            raise AssertionError(f"{what}: bytes outside the touched rectangle were written, the first in the "
                                 f"8 bytes at offset {at} ({at / GIB:.3f} GiB) of {t.numel()}")
    assert bool((t[n8:] == sentinel).all()), f"{what}: the last bytes of the buffer were written"


def check(t, expected_twin, twin, big, code, what, compare=None, sentinel=SENTINEL):
    """the stretched buffer `t` against the twin's expected buffer: the touched rectangle (a custom
    case: every block) bit for bit on the device, then the sentinel everywhere else.  When the bits
    differ the rectangle goes to the host and `compare(got, expected)` (the family's assertion, which
    may accept any NaN for a NaN) decides and words the failure."""
    import torch
    exp = _dev_bytes(expected_twin)
    if isinstance(big, BC):
        r = _rect(t, twin, big, code)
        got = r
        same = torch.equal(r, exp.view(r.shape))
    else:
        src, dst = _index(big, code)
        got, exp_sel = t[dst], exp[src]
        same = torch.equal(got, exp_sel)
    if not same:
        assert compare is not None, f"{what}: the touched rectangle differs from the expected twin"
        e = np.ascontiguousarray(expected_twin)
        if isinstance(big, BC):
            g = got.contiguous().cpu().numpy().reshape(-1).view(e.dtype)
        else:  # (the gaps between blocks keep the expected twin's bytes)
            gb = exp.clone()
            gb[src] = got
            g = gb.cpu().numpy().view(e.dtype)
        compare(g, e.reshape(-1))
    if isinstance(big, BC):
        r.fill_(sentinel)
    else:
        t[dst] = sentinel
    assert_sentinel(t, what, sentinel)


# ------------------------------------------------------------------ host checks before a launch
def tile_part(ops):
    """the costa_tile_op_t records of a plain, tri or scaled op array"""
    return ops["op"] if "op" in (ops.dtype.names or ()) else ops


def check_footprints(ops, ta, tc, src, dst, what):
    """(a) every op's source and destination footprint lies inside its allocation; src / dst =
    (first byte, one past the last byte).  Python integers throughout."""
    for x, o in enumerate(tile_part(ops)):
        nf, ns, lds, ldd = (int(o[k]) for k in ("nf", "ns", "lds", "ldd"))
        if nf <= 0 or ns <= 0:
            continue
        tr = int(o["flags"]) & 1
        s0, d0 = int(o["src"]), int(o["dst"])
        s1 = s0 + nbytes(ta, (ns - 1) * lds) + -(-nf * QB[ta] // 4)
        run, runs = (ns, nf) if tr else (nf, ns)
        d1 = d0 + nbytes(tc, (runs - 1) * ldd) + -(-run * QB[tc] // 4)
        assert lds > 0 and ldd > 0, f"{what}: op {x} leading dimensions {lds}, {ldd}"
        assert src[0] <= s0 and s1 <= src[1], (f"{what}: op {x} reads [{s0:#x}, {s1:#x}) outside the source "
                                               f"allocation [{src[0]:#x}, {src[1]:#x})")
        assert dst[0] <= d0 and d1 <= dst[1], (f"{what}: op {x} writes [{d0:#x}, {d1:#x}) outside the "
                                               f"destination allocation [{dst[0]:#x}, {dst[1]:#x})")


def grid_offsets(ops, bf, bs):
    """per sub-tile of every op on a bf x bs grid: (source, destination) offset in ELEMENTS of the
    sub-tile's first element from the op's first element, as the kernels compute them
    (s0 * lds + f0; s0 * ldd + f0, transposing ops f0 * ldd + s0)"""
    out = []
    for o in tile_part(ops):
        nf, ns, lds, ldd = (int(o[k]) for k in ("nf", "ns", "lds", "ldd"))
        tr = int(o["flags"]) & 1
        for s0 in range(0, ns, bs):
            for f0 in range(0, nf, bf):
                out.append((s0 * lds + f0, f0 * ldd + s0 if tr else s0 * ldd + f0))
    return out


_SKEW = {4: {False: (32, 512), True: (64, 256)}, 8: {False: (64, 128)}}  # tile_kernels.hip skew_shape


def plain_lists(costa, code, ops, kind="local", device=None):
    """the executor's work lists of a plain op list: (launch variants, [(source, destination) offsets in
    elements of every sub-tile item of the shaped and skew classes], ordered ops, meta)"""
    import tile_lists
    w = costa.work_export(code, ops, kind, device)
    m = w.meta
    vs = tile_lists.variants(code, ops, kind)
    t = tile_lists.NAMES[int(code)]
    E = QB[int(code)] // 4
    spans = []
    for lo, n, names in ((0, m["n_large"], ("large", "large_tr", "large_tr_full", "small_tr")),
                         (m["n_large"], m["n_medium"], ("medium_tr", "medium_tr_full", "small32_tr"))):
        if n > 0:
            (v,) = [x for x in names if x in vs]
            spans.append((lo, n) + tile_lists._DIMS[t][v])
    if m["n_skew"] > 0:
        spans.append((m["n_large"] + m["n_medium"], m["n_skew"]) + _SKEW[E]["skew_wide" in vs])
    offs = []
    for lo, n, bf, bs in spans:
        for item in w.work[lo:lo + n]:
            o = w.ordered[int(item) >> 32]
            q = int(item) & 0xFFFFFFFF
            nf, ns, lds, ldd = (int(o[k]) for k in ("nf", "ns", "lds", "ldd"))
            nbf = -(-nf // bf)
            f0, s0 = q % nbf * bf, q // nbf * bs
            assert f0 < nf and s0 < ns, "a work item outside its op"
            offs.append((s0 * lds + f0, f0 * ldd + s0 if int(o["flags"]) & 1 else s0 * ldd + f0))
    real = np.ones(w.ordered.size, bool)  # (a destination-block group's header record is no op)
    real[w.work[m["n_large"] + m["n_medium"] + m["n_skew"]:].astype(np.int64)] = False
    return vs, offs, w.ordered[real], m


def crossing(offsets, rule, ta, tc, side, what):
    """(b) on each stretched side, sub-tiles start on both sides of the rule's threshold.
    -> {side: largest offset in elements}"""
    out = {}
    for k, (name, code) in enumerate((("src", ta), ("dst", tc))):
        if side not in (name, "both"):
            continue
        thr = threshold_elems(rule, code)
        v = [o[k] for o in offsets]
        assert v, f"{what}: the lists hold no sub-tile item"
        assert max(v) >= thr, f"{what}: no {name} sub-tile starts {thr} elements or more into its op (max {max(v)})"
        assert any(0 < x < thr for x in v), f"{what}: no {name} sub-tile starts below the threshold"
        out[name] = max(v)
    return out


def arena_crossing(ops, ta, tc, lo_src, lo_dst, what):
    """(b) for the two-arena custom pair: ops start on both sides of 2^32 bytes from the lowest block
    address of their side"""
    o = tile_part(ops)
    for name, first, lo in (("src", [int(x) for x in o["src"]], lo_src), ("dst", [int(x) for x in o["dst"]], lo_dst)):
        assert min(first) >= lo and max(first) - lo >= BYTE_RULE and min(first) - lo < BYTE_RULE, \
            f"{what}: the {name} ops do not straddle 2^32 bytes from the lowest block"


# ------------------------------------------------------------------ element maps (CPU tests)
def element_address(case, base, code, i, j):
    """closed form, from the layout parameters alone: the byte address of element (i, j) (0-based in
    the matrix the layout describes, numpy int64 arrays) of a one-rank layout at `base`"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    if isinstance(case, BC):
        assert case.pm == case.pn == 1
        lld = np.int64(case.sizes(1)[0])
        r, c = i + (case.ia - 1), j + (case.ja - 1)  # one rank: local = global
        e = c * lld + r if case.ord == "C" else r * lld + c
        return np.int64(base) + e * QB[code] // 4
    twin = case.twin if isinstance(case, TwoArena) else case
    rs, cs = np.asarray(twin.rowsplit, np.int64), np.asarray(twin.colsplit, np.int64)
    nbr, nbc = twin.owners.shape
    first = np.zeros((nbr, nbc), np.int64)
    lds = np.ones((nbr, nbc), np.int64)
    if isinstance(case, TwoArena):
        for bi, bj, _, pos, ld, _ in case.blocks:
            first[bi, bj], lds[bi, bj] = pos, ld
    else:
        for bi, bj, off, ld in twin._blocks(1)[0][0]:
            first[bi, bj], lds[bi, bj] = off, ld
    bi = np.searchsorted(rs, i, side="right") - 1
    bj = np.searchsorted(cs, j, side="right") - 1
    r, c = i - rs[bi], j - cs[bj]
    e = first[bi, bj] + (c * lds[bi, bj] + r if twin.ord == "C" else r * lds[bi, bj] + c)
    return np.int64(base) + e * QB[code] // 4


def expand_ops(ops, ta, tc, keep=None):
    """every element an op list moves, as numpy int64 arrays (destination address, source address,
    op index, f, s); `keep(op record) -> nf x ns bool` drops elements (edge ops)"""
    d, s_, idx, ff, ss = [], [], [], [], []
    tiles = tile_part(ops)
    for x, o in enumerate(tiles):
        nf, ns = int(o["nf"]), int(o["ns"])
        if nf <= 0 or ns <= 0:
            continue
        f, s = np.meshgrid(np.arange(nf, dtype=np.int64), np.arange(ns, dtype=np.int64), indexing="ij")
        lds, ldd = np.int64(o["lds"]), np.int64(o["ldd"])
        so = s * lds + f
        do = f * ldd + s if int(o["flags"]) & 1 else s * ldd + f
        k = np.ones(f.shape, bool) if keep is None else keep(ops[x])
        d.append((np.int64(o["dst"]) + do * QB[tc] // 4)[k])
        s_.append((np.int64(o["src"]) + so * QB[ta] // 4)[k])
        idx.append(np.full(int(k.sum()), x, np.int64))
        ff.append(f[k])
        ss.append(s[k])
    if not d:
        z = np.zeros(0, np.int64)
        return z, z, z, z, z
    return tuple(np.concatenate(v) for v in (d, s_, idx, ff, ss))


# ------------------------------------------------------------------ the stretched cases of the tests
F32, F64, C64, C128, I32, H16, BF16, E4M3, E5M2 = 0, 1, 2, 3, 4, 5, 6, 7, 8
TNAMES = {0: "f32", 1: "f64", 2: "c64", 3: "c128", 4: "i32", 5: "f16", 6: "bf16", 7: "e4m3", 8: "e5m2",
          9: "e2m1", 10: "e2m3", 11: "e3m2"}


@dataclasses.dataclass
class Spec:
    """one stretched case: `family` names the entry point and the reference; a_twin / c_twin are the
    ordinary cases, `rule` / `side` what is stretched and how far; `mode` the planner (plain) or the
    list builder (custom) the case runs under; `extra` family arguments (uplo, k, ...)"""
    family: str
    ta: int
    tc: int
    op: str
    alpha: complex
    beta: complex
    a_twin: object
    c_twin: object
    rule: str = "bytes"
    side: str = "both"
    mode: int = 0
    extra: dict = dataclasses.field(default_factory=dict)
    tag: str = ""
    frac: float = 0.75

    @property
    def id(self):
        t = TNAMES[self.ta] if self.ta == self.tc else f"{TNAMES[self.ta]}-{TNAMES[self.tc]}"
        return "-".join(x for x in (self.family, t, self.op, self.tag, self.rule, self.side, f"m{self.mode}") if x)

    def big(self):
        """(stretched A case, stretched C case); a side that is not stretched stays the twin"""
        if isinstance(self.a_twin, Custom):
            gap = threshold_elems("bytes", self.ta) + STEP
            return TwoArena(self.a_twin, gap), TwoArena(self.c_twin, threshold_elems("bytes", self.tc) + STEP)
        if self.rule == "fp6ld":  # a packed FP6 side whose 3 * ld passes 2^31 (its byte pitch is 3 * ld / 4)
            lld = (1 << 31) // 3 + 1
            return (with_lld(self.a_twin, lld) if self.side == "src" else self.a_twin,
                    with_lld(self.c_twin, lld) if self.side == "dst" else self.c_twin)
        a = stretched(self.a_twin, threshold_elems(self.rule, self.ta), "src", self.frac) if self.side in ("src", "both") else self.a_twin
        c = stretched(self.c_twin, threshold_elems(self.rule, self.tc), "dst", self.frac) if self.side in ("dst", "both") else self.c_twin
        return a, c


size_bytes = big_bytes


def _dims(m, n, op):
    return (n, m) if op != "N" else (m, n)


def _scalars(code, nonzero):
    """alpha, beta = 1, 0, or both nonzero"""
    if not nonzero:
        return 1, 0
    if code in (C64, C128):
        return 0.75 - 0.5j, 1.25 + 0.25j
    return (3, -2) if code == I32 else (-0.5, 2.0)


def plain_specs():
    """plain transforms: every type x op x pad (aligned, odd) x block (24^2, 128^2) x scalars (1, 0 /
    both nonzero), the planner (host 0, GPU 2) alternating so that every type and op meets both; the
    element rule (4-byte types, one side at a time); one row-major side.  1100 x 1040: a 4-byte skew
    sub-tile is 512 columns of the source, and a granule-split copy op keeps every 16th column, so
    smaller matrices have no sub-tile in their last quarter."""
    out = []
    m, n = 1100, 1040
    for code in (F32, F64, C64, C128, I32):
        for io, op in enumerate(("N", "C" if code in (C64, C128) else "T")):
            for pad in (0, 1):
                for ib, mb in enumerate((24, 128)):
                    for nz in (0, 1):
                        al, be = _scalars(code, nz)
                        am, an = _dims(m, n, op)
                        out.append(Spec("plain", code, code, op, al, be, BC(am, an, mb, mb, lld_pad=pad),
                                        BC(m, n, mb, mb, lld_pad=pad), mode=(0, 2)[(io + pad + ib + nz) % 2],
                                        tag=f"b{mb}-pad{pad}-{('ab10', 'abxy')[nz]}"))
    for code in (F32, I32):
        for op, side in (("N", "src"), ("T", "dst"), ("T", "src"), ("N", "dst")):
            if code == I32 and (op, side) in (("T", "src"), ("N", "dst")):
                continue
            am, an = _dims(m, n, op)
            al, be = _scalars(code, side == "src")
            # ('T' into a compact target is all destination-block groups, whose ops have no sub-tiles:
            # a target pitch past the group budget keeps the transposing shapes)
            amb, pad, cpad = (128, 0, 8192) if (op, side) == ("T", "src") else (24, 1, 0)
            out.append(Spec("plain", code, code, op, al, be, BC(am, an, amb, amb, lld_pad=pad),
                            BC(m, n, 128, 128, lld_pad=cpad),
                            rule="elems", side=side, mode=2 if side == "src" else 0, tag=f"b{amb}-b128"))
    for op in ("N", "T"):  # row-major storage on the source side, a sub-matrix on the target side
        am, an = _dims(m, n, op)
        out.append(Spec("plain", F64, F64, op, -0.5, 2.0, BC(am, an, 24, 24, ord="R"),
                        BC(m + 9, n + 11, 128, 128, ia=5, ja=7, subm=m, subn=n, lld_pad=1), mode=2, tag="rowmajor-sub"))
    return out


def custom_specs():
    """the two-arena custom pair: ragged blocks of 8-60, fp32, host and GPU list builder; a lone strip
    of 3 rows and one of 2 columns in C, whose blocks run as wavefront pieces beside the groups"""
    def edges(seed, n):
        r = np.random.default_rng(seed)
        s = [0]
        while s[-1] < n:
            s.append(min(n, s[-1] + int(r.integers(8, 61))))
        return s
    out = []
    m, n = 203, 157
    for op in ("N", "T"):
        for mode in (0, 2):
            am, an = _dims(m, n, op)
            ars, acs, crs, ccs = edges(11, am), edges(12, an), edges(13, m), edges(14, n)
            crs, ccs = [0, 3] + crs[1:], [0, 2] + ccs[1:]
            a = Custom(ars, acs, np.zeros((len(ars) - 1, len(acs) - 1), np.int32), ld_pad=1, gap=3)
            c = Custom(crs, ccs, np.zeros((len(crs) - 1, len(ccs) - 1), np.int32), gap=4)
            al, be = _scalars(F32, (op == "T") == (mode == 0))
            out.append(Spec("custom", F32, F32, op, al, be, a, c, mode=mode, tag="arenas"))
    return out


def _one(m, n, op, pad_a=0, pad_c=0):
    """one block per side: the strip families do not merge ops, so only an op over the whole local
    matrix has sub-tiles on both sides of a threshold"""
    am, an = _dims(m, n, op)
    return BC(am, an, am, an, lld_pad=pad_a), BC(m, n, m, n, lld_pad=pad_c)


def strip_specs():
    """the strip families on one op of 300 x 260: byte rule on both sides, and the element rule for
    the element types below 4 bytes (one case per such pair, alternating 'N' / 'T')"""
    out = []
    m, n = 300, 260

    calls = [0]

    def add(fam, ta, tc, rules=("bytes",), m=m, n=n, frac=0.75, **extra):
        calls[0] += 1
        for ir, rule in enumerate(rules):
            for op in ("N", "T"):
                a, c = _one(m, n, op, pad_a=(0, 1)[op == "T"], pad_c=0)
                # (1, 0) and both nonzero swap between 'N' and 'T' from one pair and rule to the next
                nz = (op == "T") == ((calls[0] + ir) % 2 == 0)
                al, be = (1, 0) if not nz else ((0.75 - 0.5j, 1.25 + 0.25j) if tc in (C64, C128) else (-0.5, 2.0))
                side = "both"
                if rule == "elems":  # only the sides whose elements are below 4 bytes
                    side = "both" if QB[ta] < 16 and QB[tc] < 16 else "src" if QB[ta] < 16 else "dst"
                out.append(Spec(fam, ta, tc, op, al, be, a, c, rule=rule, side=side, extra=dict(extra), frac=frac))
    add("mixed", F64, F32)
    add("mixed", F32, F64)
    add("mixed", C128, C64)
    add("half", H16, F32, ("bytes", "elems"))
    add("half", F32, H16, ("bytes", "elems"))
    add("half", BF16, BF16, ("bytes", "elems"))
    add("fp8", E4M3, E4M3, ("bytes", "elems"))
    add("fp8", F32, E5M2, ("bytes", "elems"))
    add("fp8", E4M3, F32, ("bytes", "elems"))
    add("scaled", F32, F32)
    add("scaled", BF16, BF16, ("elems",))
    add("amax", F32, F32)
    add("amax", E4M3, F32, ("elems",))
    # (the planner cuts a block the diagonal crosses into bands of 256 rows whose edge tile is at most
    # 255 columns wide: its last 64-column sub-tile starts at column 192 of 256, hence 0.72)
    add("tri", F64, F64, m=256, n=256, frac=0.72, uplo="U", k=-21)
    add("tri", F32, F32, m=256, n=256, frac=0.72, uplo="L", k=37)
    return out


def mx_specs():
    """transform_mx (FP8, packed FP4, packed FP6) and transform_block_scaled: quantise, dequantise and
    requantise on one op of 300 x 260 (even, and a multiple of 4: no byte or 3-byte group is split),
    byte rule on both sides, the element rule on the narrow sides; and FP6 with 3 * ld past 2^31"""
    out = []
    m, n = 300, 260
    FP4, E2M3, E3M2 = 9, 10, 11
    for fam, q in (("mx", E4M3), ("mx4", FP4), ("mx6", E2M3), ("bs", E5M2)):
        for kind, (ta, tc) in (("quantise", (F32, q)), ("dequantise", (q, F32)), ("requantise", (q, q))):
            for k, op in enumerate(("N", "T")):
                rule = ("bytes", "elems")[(k + (kind == "dequantise")) % 2]
                side = "both"
                if rule == "elems":
                    side = "both" if ta == tc else "src" if tc == F32 else "dst"
                a, c = _one(m, n, op, pad_a=(0, 4)[op == "T"])
                al, be = (1.0, 0.0) if op == "N" else (-0.5, 2.0) if kind == "dequantise" else (0.75, 0.0)
                out.append(Spec(fam, ta, tc, op, al, be, a, c, rule=rule, side=side, extra=dict(kind=kind)))
    # 64 x 20, one op: the packed side's leading dimension is 715.8 M elements, 537 MB a column
    out.append(Spec("mx6", E3M2, F32, "N", -0.5, 2.0, *_one(64, 20, "N"), rule="fp6ld", side="src",
                    extra=dict(kind="dequantise")))
    out.append(Spec("mx6", F32, E3M2, "T", 0.75, 0.0, *_one(64, 20, "T"), rule="fp6ld", side="dst",
                    extra=dict(kind="quantise")))
    return out


def export(costa, spec, LA, LC):
    """the op lists the call will launch and its sub-tiles' offsets, from the exports alone:
    -> (list of op arrays, [(source, destination) offsets in elements], variants / sub-tile text)"""
    fam = spec.family
    if fam in ("plain", "custom"):
        p = costa.plan_export([LA], [LC], 0, 1, [spec.op], [spec.alpha], [spec.beta])
        assert p.pack_ops.size == 0 and p.unpack_ops.size == 0
        vs, offs, ordered, _ = plain_lists(costa, spec.ta, p.local_ops)
        return [p.local_ops, ordered], offs, "+".join(sorted(vs)), p
    if fam in ("mixed", "half", "fp8"):
        p = costa.plan_export([LA], [LC], 0, 1, [spec.op], [spec.alpha], [spec.beta])
        assert p.pack_ops.size == 0 and p.unpack_ops.size == 0
        bf, bs = costa.convert_subtile(spec.ta, spec.tc)
        return [p.local_ops], grid_offsets(p.local_ops, bf, bs), f"convert {bf}x{bs}", p
    if fam in ("scaled", "amax", "mx", "mx4", "mx6", "bs"):
        p = costa.plan_export_scaled(LA, LC, 0, 1, spec.op, spec.alpha, spec.beta)
        assert p.pack_ops.size == 0 and p.unpack_scaled.size == 0
        sub = costa.block_subtile if fam == "bs" else costa.scaled_subtile if fam in ("scaled", "amax") else costa.mx_subtile
        bf, bs = sub(spec.ta, spec.tc)
        return [p.local_scaled], grid_offsets(p.local_scaled, bf, bs), f"{fam} {bf}x{bs}", p
    if fam == "tri":
        p = costa.plan_export_tri(LA, LC, 0, 1, spec.op, spec.extra["uplo"], spec.extra["k"], spec.alpha, spec.beta)
        assert p.pack_ops.size == 0 and p.unpack_ops.size == 0 and p.unpack_tri.size == 0
        bf, bs = costa.tri_subtile(spec.ta)
        offs = grid_offsets(p.local_tri, bf, bs)
        text = f"tri {bf}x{bs}"
        lists = [p.local_tri]
        if p.local_ops.size:
            vs, o2, ordered, _ = plain_lists(costa, spec.ta, p.local_ops)
            offs, text = offs + o2, text + "+" + "+".join(sorted(vs))
            lists += [p.local_ops, ordered]
        return lists, offs, text, p
    raise KeyError(fam)


def host_checks(costa, spec, a_big, c_big, a_ptr, c_ptr):
    """checks (a) and (b) of a case at the given buffer addresses; -> (layouts, variants text,
    largest offsets, plan)"""
    LA, LC = make_layout(costa, a_big, a_ptr, spec.ta), make_layout(costa, c_big, c_ptr, spec.tc)
    lists, offs, text, p = export(costa, spec, LA, LC)
    src = (a_ptr, a_ptr + size_bytes(a_big, spec.ta))
    dst = (c_ptr, c_ptr + size_bytes(c_big, spec.tc))
    for ops in lists:
        check_footprints(ops, spec.ta, spec.tc, src, dst, spec.id)
    if spec.family == "custom":
        assert text.startswith("cblock_") and text.endswith("+pieces"), f"{spec.id}: {text}: groups and pieces wanted"
        arena_crossing(lists[1], spec.ta, spec.tc, a_ptr, c_ptr, spec.id)
        far = {"src": max(int(x) for x in lists[1]["src"]) - a_ptr, "dst": max(int(x) for x in lists[1]["dst"]) - c_ptr}
    elif spec.rule == "fp6ld":
        key = {"src": "lds", "dst": "ldd"}[spec.side]
        ld = [int(x) for x in tile_part(lists[0])[key]]
        assert ld and all(3 * x >= 1 << 31 and x < 1 << 31 for x in ld), f"{spec.id}: 3 * {key} stays below 2^31"
        far = {spec.side + " 3*ld": 3 * max(ld)}
    else:
        far = crossing(offs, spec.rule, spec.ta, spec.tc, spec.side, spec.id)
    return (LA, LC), text, far, p
