"""Shared by tests/test_gpu_plan_cache.py: transform-level calls through the plan cache
(engine.cpp get_plan / upload_scalars) inside guarded arenas, every call compared with the CPU
oracle over the whole arena.

A `Variant` is one call: the entry point, the element pair, one or more (A case, C case, op, alpha,
beta) pairs at byte offsets inside the arenas, the mask or the vectors where they apply.  A `Rig`
owns one arena for A and one for C, device-resident, pageable or page-locked.  Rig.run(variant, seed)
  fills both arenas with the guard pattern and seeded data (finite values only),
  computes the expected image of the C arena with the family's expected_* helper,
  makes the call, and compares the whole C arena byte for byte (guard zones included; the A arena
  must come back unchanged), then returns the deltas of plan_hits, plan_misses and device_plans.

Arena rule: all variants of one test that a wrong cache could confuse live in the same two arenas,
each sized for the largest variant plus GUARD bytes on both sides, so a plan replayed for the wrong
call stays inside memory the test owns and shows up as a byte mismatch.
"""
from dataclasses import dataclass, field

import numpy as np

import fp8_common as fc
import half_common as hc
import oracle
import scaled_common as sc
from amax_common import expected_transform_amax
from casegen import BC, Custom
from tri_common import distribute, keep_mask

F, D, CF, CD, I32, H16, BF16, E4M3, E5M2 = 0, 1, 2, 3, 4, 5, 6, 7, 8
ESIZE = {F: 4, D: 8, CF: 8, CD: 16, I32: 4, H16: 2, BF16: 2, E4M3: 1, E5M2: 1}
GUARD = 64 << 10
make_layout = fc.make_layout  # (knows every element code)


def pattern(n):
    """n bytes of the guard pattern (a fixed function of the position)"""
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761) >> np.uint64(13)) & np.uint64(0xFF)).astype(np.uint8)


def gen(code, seed, n):
    """n finite elements of `code` (raw bits for the 1- and 2-byte types)"""
    if code in (CF, CD, I32):
        return oracle.gen(code, seed, 0, n)
    return sc.gen(code, seed, n)


@dataclass
class Moved(Custom):
    """a Custom layout whose blocks sit elsewhere in the buffer: block t (row-major block order) moves
    up by shifts[0] + ... + shifts[t % len] elements, each block by a different amount, and the two
    blocks of `swap` (equal extents) trade places"""
    shifts: tuple = ()
    swap: tuple = ()

    def _blocks(self, P):
        per, size = super()._blocks(P)
        assert P == 1
        out, add = [], 0
        for t, (i, j, off, ld) in enumerate(per[0]):
            if self.shifts:
                add += self.shifts[t % len(self.shifts)]
            out.append((i, j, off + add, ld))
        if self.swap:
            x, y = self.swap
            (ix, jx, ox, lx), (iy, jy, oy, ly) = out[x], out[y]
            ext = [(self.rowsplit[i + 1] - self.rowsplit[i], self.colsplit[j + 1] - self.colsplit[j])
                   for i, j in ((ix, jx), (iy, jy))]
            assert ext[0] == ext[1] and lx == ly, "swapped blocks must have equal extents"
            out[x], out[y] = (ix, jx, oy, lx), (iy, jy, ox, ly)
        return [out], [size[0] + add]


@dataclass
class Pair:
    a_case: object
    c_case: object
    op: str = "N"
    alpha: complex = 1
    beta: complex = 0
    a_off: int = 0  # byte offsets of the pair's buffers inside the arenas' payloads
    c_off: int = 0


@dataclass
class Variant:
    pairs: list
    ta: int = D
    tc: int = None
    entry: str = "transform"  # transform | batch | tri | scaled | amax
    uplo: str = "U"
    k: int = 0
    rows: bool = True    # scaled / amax: a row_scale vector is given
    cols: bool = True
    use_async: bool = False  # the entry point's _async form on a torch stream, synchronised after
    swapped: bool = False    # the source lives in the rig's C arena and the target in its A arena
    host_mode: int = None    # set_host_staging(host_mode) around the call
    name: str = ""
    layouts: object = field(default=None, repr=False)

    def __post_init__(self):
        if self.tc is None:
            self.tc = self.ta
        if isinstance(self.pairs, Pair):
            self.pairs = [self.pairs]


def one(a_case, c_case, op="N", alpha=1, beta=0, a_off=0, c_off=0, **kw):
    """a Variant of one pair"""
    return Variant([Pair(a_case, c_case, op, alpha, beta, a_off, c_off)], **kw)


def bc_pair(op, m, n, a_blk=(32, 48), c_blk=(40, 24), a_kw=None, c_kw=None):
    """(A case, C case): block-cyclic, C m x n and A of op's shape"""
    am, an = (n, m) if op != "N" else (m, n)
    return BC(am, an, *a_blk, **(a_kw or {})), BC(m, n, *c_blk, **(c_kw or {}))


def buf_bytes(case, code):
    return case.buf_elems(0, 1) * ESIZE[code]


def payload(variants):
    """(A payload, C payload) bytes that hold every variant of the list"""
    a = c = 0
    for v in variants:
        for p in v.pairs:
            ea, ec = p.a_off + buf_bytes(p.a_case, v.ta), p.c_off + buf_bytes(p.c_case, v.tc)
            if v.swapped:
                ea, ec = ec, ea
            a, c = max(a, ea), max(c, ec)
    return a, c


# ------------------------------------------------------------------ expected values
def expected_plain(ta, tc, p, a, c):
    if ta == tc and ta in oracle.NP:
        e = c.copy()
        oracle.transform(tc, p.op, p.alpha, p.beta, p.a_case.geom(1), [a], p.c_case.geom(1), [e])
        return e
    if ta in oracle.NP and tc in oracle.NP:  # FLOAT <-> DOUBLE: the source converted first
        e = c.copy()
        oracle.transform(tc, p.op, p.alpha, p.beta, p.a_case.geom(1), [a.astype(oracle.NP[tc])],
                         p.c_case.geom(1), [e])
        return e
    mod = hc if H16 in (ta, tc) or BF16 in (ta, tc) else fc
    return mod.expected_transform(ta, tc, p.op, p.alpha, p.beta, p.a_case, p.c_case, a, c)


def expected_pair(v, p, a, c, r, cs):
    """the whole expected C buffer of one pair of variant v"""
    if v.entry in ("scaled", "amax"):
        return sc.expected_transform(v.ta, v.tc, p.op, p.alpha, p.beta, p.a_case, p.c_case, a, c, r, cs)
    full = expected_plain(v.ta, v.tc, p, a, c)
    if v.entry != "tri":
        return full
    m, n = p.c_case.shape()
    keep = distribute(keep_mask(m, n, v.uplo, v.k).astype(np.float64), p.c_case, 1)[0]
    return np.where(keep == 1, full, c)


# ------------------------------------------------------------------ arenas
class Arena:
    """guard | payload | guard in one allocation; the payload starts on a 4096-byte boundary"""

    def __init__(self, payload_bytes, residency="device"):
        import torch
        self.residency = residency
        n = GUARD + 4096 + payload_bytes + GUARD
        if residency == "device":
            self.t = torch.empty(n, dtype=torch.uint8, device="cuda")
            addr = self.t.data_ptr()
        elif residency == "pinned":
            self.t = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            self.h = self.t.numpy()
            addr = self.h.ctypes.data
        else:
            assert residency == "pageable"
            self.h = np.empty(n, np.uint8)
            addr = self.h.ctypes.data
        self.size = n
        self.lead = GUARD + (-(addr + GUARD)) % 4096
        self.base = addr + self.lead
        self.room = n - self.lead - GUARD
        assert self.room >= payload_bytes and self.base % 4096 == 0
        self._pattern = pattern(n)
        self._pattern.setflags(write=False)

    def fresh(self):
        return self._pattern.copy()

    def put(self, image):
        import torch
        assert image.size == self.size and image.dtype == np.uint8
        if self.residency == "device":
            self.t.copy_(torch.from_numpy(image))
            torch.cuda.synchronize()
        else:
            self.h[:] = image

    def get(self):
        import torch
        if self.residency == "device":
            torch.cuda.synchronize()
            return self.t.cpu().numpy()
        return self.h.copy()

    def region(self, image, off, code, count):
        """`count` elements of `code` at payload offset `off` of an arena image (a view)"""
        lo = self.lead + off
        assert off >= 0 and off + count * ESIZE[code] <= self.room, "a variant outside its arena"
        return image[lo:lo + count * ESIZE[code]].view(sc.NPT.get(code, oracle.NP.get(code)))


def assert_image(got, exp, arena, what):
    if got.tobytes() == exp.tobytes():
        return
    bad = np.flatnonzero(got != exp)
    raise AssertionError(f"{what}: {bad.size} bytes of the arena differ from the oracle's, first at payload "
                         f"offset {int(bad[0]) - arena.lead}, last at {int(bad[-1]) - arena.lead}")


@dataclass
class Delta:
    hits: int
    misses: int
    device_plans: int

    def __iter__(self):
        return iter((self.hits, self.misses))


MISS, HIT = (0, 1), (1, 0)  # tuple(delta) of a call that planned / that replayed


def stats_delta(costa, st0):
    st1 = costa.get_stats()
    return Delta(*(int(st1[k] - st0[k]) for k in ("plan_hits", "plan_misses", "device_plans")))


class Rig:
    def __init__(self, costa, variants, residency="device", slack=0):
        a, c = payload(variants)
        self.costa = costa
        self.A = Arena(a + slack, residency)
        self.C = Arena(c + slack, residency)
        self.comm = costa.Comm.self(0)
        self.residency = residency

    def arenas(self, v):
        return (self.C, self.A) if v.swapped else (self.A, self.C)

    def layouts(self, v):
        """the variant's layout handles, built once and kept (forget() closes them)"""
        if v.layouts is None or v.layouts[0] is not self:
            src, dst = self.arenas(v)
            As = [make_layout(self.costa, p.a_case, 0, src.base + p.a_off, 1, v.ta) for p in v.pairs]
            Cs = [make_layout(self.costa, p.c_case, 0, dst.base + p.c_off, 1, v.tc) for p in v.pairs]
            v.layouts = (self, As, Cs)
        return v.layouts[1], v.layouts[2]

    def forget(self, v):
        if v.layouts is not None:
            for L in v.layouts[1] + v.layouts[2]:
                L.close()
            v.layouts = None

    # ---- data and expected values
    def fill(self, v, seed, a_img, c_img):
        """seeded data into the variant's regions of the two arena images"""
        src, dst = self.arenas(v)
        for t, p in enumerate(v.pairs):
            na, nc = p.a_case.buf_elems(0, 1), p.c_case.buf_elems(0, 1)
            src.region(a_img, p.a_off, v.ta, na)[:] = gen(v.ta, 1000 * seed + 2 * t + 1, na)
            dst.region(c_img, p.c_off, v.tc, nc)[:] = gen(v.tc, 1000 * seed + 2 * t + 2, nc)

    def expect(self, v, a_img, exp, vec=None, times=1):
        """the oracle's result of `times` calls of v, applied to the target arena image `exp`"""
        src, dst = self.arenas(v)
        vec = vec or {}
        for _ in range(times):
            for p in v.pairs:
                na, nc = p.a_case.buf_elems(0, 1), p.c_case.buf_elems(0, 1)
                a = src.region(a_img, p.a_off, v.ta, na).copy()
                c = dst.region(exp, p.c_off, v.tc, nc)
                c[:] = expected_pair(v, p, a, c.copy(), vec.get("r"), vec.get("c"))

    def images(self, v, seed, times=1):
        """(source arena image, target arena image before, expected after `times` calls, vectors) of
        variant v on seeded data"""
        src, dst = self.arenas(v)
        a_img, c_img = src.fresh(), dst.fresh()
        self.fill(v, seed, a_img, c_img)
        vec = {}
        if v.entry in ("scaled", "amax"):
            ct = sc.ctype(v.ta, v.tc)
            m, n = v.pairs[0].c_case.shape()
            vec["r"] = sc.scales(m, 10 * seed + 1, ct) if v.rows else None
            vec["c"] = sc.scales(n, 10 * seed + 2, ct) if v.cols else None
        exp = c_img.copy()
        self.expect(v, a_img, exp, vec, times)
        if v.entry == "amax":
            p = v.pairs[0]
            a = src.region(a_img, p.a_off, v.ta, p.a_case.buf_elems(0, 1)).copy()
            vec["ra"], vec["ca"] = expected_transform_amax(v.ta, v.tc, p.op, p.a_case, p.c_case, a,
                                                           np.zeros(m, ct), np.zeros(n, ct))
        return a_img, c_img, exp, vec

    # ---- the call
    def call(self, v, vec=None, stream=None, dev_vec=None):
        """the variant's entry point; `stream` selects the _async form.  Device copies of the vectors
        go into dev_vec (they must outlive an asynchronous call)."""
        import torch
        costa = self.costa
        As, Cs = self.layouts(v)
        p = v.pairs[0]
        keep = dev_vec if dev_vec is not None else {}
        if v.entry in ("scaled", "amax"):
            for k in ("r", "c"):
                keep[k] = None if vec[k] is None else torch.from_numpy(vec[k]).cuda()
        if v.host_mode is not None:
            costa.set_host_staging(v.host_mode)
        try:
            if v.entry == "transform" and stream is None:
                costa.transform(As[0], Cs[0], self.comm, p.op, p.alpha, p.beta)
            elif v.entry == "transform":
                costa.transform_async(As[0], Cs[0], self.comm, p.op, p.alpha, p.beta, stream=stream)
            elif v.entry == "batch":
                fn = costa.transform_batch if stream is None else costa.transform_batch_async
                kw = {} if stream is None else {"stream": stream}
                fn(As, Cs, self.comm, [q.op for q in v.pairs], [q.alpha for q in v.pairs],
                   [q.beta for q in v.pairs], **kw)
            elif v.entry == "tri" and stream is None:
                costa.transform_tri(As[0], Cs[0], self.comm, p.op, v.uplo, v.k, p.alpha, p.beta)
            elif v.entry == "tri":
                costa.transform_tri_async(As[0], Cs[0], self.comm, p.op, v.uplo, v.k, p.alpha, p.beta,
                                          stream=stream)
            elif v.entry == "scaled":
                costa.transform_scaled(As[0], Cs[0], self.comm, p.op, p.alpha, p.beta, keep["r"], keep["c"],
                                       stream=stream)
            elif v.entry == "amax":
                ct = sc.ctype(v.ta, v.tc)
                m, n = p.c_case.shape()
                keep["ra"] = torch.from_numpy(np.zeros(m, ct)).cuda()
                keep["ca"] = torch.from_numpy(np.zeros(n, ct)).cuda()
                costa.transform_amax(As[0], Cs[0], self.comm, p.op, p.alpha, p.beta, keep["r"], keep["c"],
                                     keep["ra"], keep["ca"], stream=stream)
            else:
                raise KeyError(v.entry)
        finally:
            if v.host_mode is not None:
                costa.set_host_staging(1)
        return keep

    def run(self, v, seed, what=""):
        """one call of v on fresh seeded data, checked against the oracle over both whole arenas;
        returns the Delta of the plan-cache counters over the call"""
        import torch
        what = what or v.name or v.entry
        src, dst = self.arenas(v)
        a_img, c_img, exp, vec = self.images(v, seed)
        src.put(a_img)
        dst.put(c_img)
        st0 = self.costa.get_stats()
        stream = torch.cuda.Stream() if v.use_async else None
        keep = self.call(v, vec, stream)
        delta = stats_delta(self.costa, st0)
        if stream is not None:
            stream.synchronize()
        assert_image(dst.get(), exp, dst, f"{what} (seed {seed}): C")
        assert_image(src.get(), a_img, src, f"{what} (seed {seed}): A")
        if v.entry == "amax":
            for k, name in (("ra", "row_amax"), ("ca", "col_amax")):
                assert keep[k].cpu().numpy().tobytes() == vec[k].tobytes(), f"{what} (seed {seed}): {name}"
        return delta
