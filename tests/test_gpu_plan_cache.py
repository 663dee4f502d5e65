"""GPU: the plan cache (engine.cpp get_plan / upload_scalars) at transform level.  In steady state
every caller repeats a layout pair, so every result reaches users through a replayed `cached_plan`:
device op and work lists with absolute addresses baked in, the scale kinds (not the values) in the
op flags, and for host-resident layouts a staging buffer or a pipeline.  These tests write the
replay contract down: what makes a call a hit, which attributes tell two calls apart, what a hit
picks up anew (data, scalar values, vectors), eviction at 16 plans, and stream order between calls
that share a plan.

Every comparison is byte equality of the whole C arena (guard zones included) with the CPU oracle's
image, on finite data; see plan_cache_common for the harness and the arena rule.  Each test uses a
geometry of its own (the `m` of its block-cyclic pair), so its hit / miss deltas are its own even
when an arena lands on an address an earlier test used.
"""
import numpy as np
import pytest

import oracle
import scaled_common as sc
from plan_cache_common import (BF16, CD, CF, D, E4M3, E5M2, ESIZE, F, H16, HIT, I32, MISS, Moved, Pair, Rig,
                               Variant, assert_image, bc_pair, buf_bytes, one, stats_delta)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu(costa):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return costa


def custom_pair(op, m, n, seed, a_kw=None, c_kw=None):
    """(A, C) custom layouts on ragged grids, every block its own buffer (the cblock path)"""
    from cases import _edges
    am, an = (n, m) if op != "N" else (m, n)
    ars, acs = _edges(seed, am, 8, 60), _edges(seed + 1, an, 8, 60)
    crs, ccs = _edges(seed + 2, m, 30, 120), _edges(seed + 3, n, 30, 120)
    za = np.zeros((len(ars) - 1, len(acs) - 1), np.int32)
    zc = np.zeros((len(crs) - 1, len(ccs) - 1), np.int32)
    return Moved(ars, acs, za, gap=1, **(a_kw or {})), Moved(crs, ccs, zc, gap=1, **(c_kw or {}))


# ------------------------------------------------------------------ 1. a hit is a replay, and right
def _representatives(m):
    """the representative calls, on geometries keyed by m"""
    n = 157
    reps = {
        "f64-T": one(*bc_pair("T", m, n), "T", 0.75, -1.5, ta=D),
        "c128-C": one(*bc_pair("C", m + 1, n), "C", 0.75 - 0.5j, 1.25 + 0.25j, ta=CD),
        "f64-f32": one(*bc_pair("T", m + 2, n), "T", 0.75, -1.5, ta=D, tc=F),
        "f32-bf16": one(*bc_pair("T", m + 3, n), "T", 0.75, -1.5, ta=F, tc=BF16),
        "f32-e4m3": one(*bc_pair("T", m + 4, n), "T", 0.75, -1.5, ta=F, tc=E4M3),
        "tri-f64-U-k1": one(*bc_pair("T", m + 5, n), "T", 0.75, -1.5, ta=D, entry="tri", uplo="U", k=1),
        "scaled-f32": one(*bc_pair("T", m + 6, n), "T", 0.75, -1.5, ta=F, entry="scaled"),
        "amax-f32-e4m3": one(*bc_pair("T", m + 7, n), "T", 0.75, -1.5, ta=F, tc=E4M3, entry="amax"),
        "cblock-f64": one(*custom_pair("T", m + 8, n, 0x9C0), "T", 0.75, -1.5, ta=D),
    }
    a0, c0 = bc_pair("T", m + 9, n)
    a1, c1 = bc_pair("N", m + 10, 131, (24, 40), (16, 56))
    ra, rc = 256 + buf_bytes(a0, D), 256 + buf_bytes(c0, D)
    reps["batch-2"] = Variant([Pair(a0, c0, "T", 0.75, -1.5), Pair(a1, c1, "N", 2.0, 0.5, ra - ra % 256, rc - rc % 256)],
                              ta=D, entry="batch")
    return reps


REPS = sorted(_representatives(203))


def _replay(rig, v, first=MISS):
    """one planning call, then three replays, each on new data in the same buffers"""
    assert tuple(rig.run(v, 1)) == first, "the first call plans exactly once"
    for seed in (2, 3, 4):
        assert tuple(rig.run(v, seed)) == HIT, f"call {seed} replays: one hit, no miss"


@pytest.mark.parametrize("rep", REPS)
def test_hit_replays_with_new_data(gpu, rep):
    """the first call is one miss, the next three one hit each, with new data written into the same A
    and C buffers before each call; every result equals the oracle's"""
    v = _representatives(203)[rep]
    _replay(Rig(gpu, [v]), v)


@pytest.mark.parametrize("rep", REPS)
def test_hit_replays_async_form(gpu, rep):
    """the same through the entry points' _async forms on a torch stream (amax and scaled: their
    stream argument)"""
    v = _representatives(303)[rep]
    v.use_async = True
    _replay(Rig(gpu, [v]), v)


HOST_REPS = ["f64-T", "c128-C", "batch-2", "cblock-f64", "tri-f64-U-k1"]


@pytest.mark.parametrize("residency,mode", [("pageable", 1), ("pageable", 0), ("pinned", 1), ("pinned", 0)])
@pytest.mark.parametrize("rep", HOST_REPS)
def test_hit_replays_host_resident(gpu, rep, residency, mode):
    """host-resident layouts, pipelined (1) and mirror (0) staging, pageable and page-locked: the
    cached staging buffer or pipeline picks up the new data of every call"""
    v = _representatives(403 + 20 * mode + (40 if residency == "pinned" else 0))[rep]
    v.host_mode = mode
    _replay(Rig(gpu, [v], residency), v)


# ------------------------------------------------------------------ 2. scalars on a hit
SCALAR_TYPES = [(D, D), (CF, CF), (F, E4M3)]
SCALAR_IDS = ["f64", "c64", "f32-e4m3"]


@pytest.mark.parametrize("ta,tc", SCALAR_TYPES, ids=SCALAR_IDS)
def test_scalar_values_change_on_a_hit(gpu, ta, tc):
    """same plan, same kinds, other values: a hit that uses the new values"""
    cx = ta == CF
    steps = [(2 + 1j, 0.5 - 0.25j), (3 - 2j, -1.25 + 1j), (3 - 2j, -1.25 + 1j), (2 + 1j, -1.25 + 1j)] if cx else \
        [(2, 0.5), (3, -1.25), (3, -1.25), (2, -1.25)]
    a_case, c_case = bc_pair("T", 211 + ta, 157)
    v = one(a_case, c_case, "T", ta=ta, tc=tc)
    rig = Rig(gpu, [v])
    for t, (alpha, beta) in enumerate(steps):
        v.pairs[0].alpha, v.pairs[0].beta = alpha, beta
        assert tuple(rig.run(v, t + 1, f"alpha {alpha} beta {beta}")) == (MISS if t == 0 else HIT)


@pytest.mark.parametrize("ta,tc", SCALAR_TYPES, ids=SCALAR_IDS)
def test_scalar_kind_transitions(gpu, ta, tc):
    """every kind transition BITCOPY / ALPHA / AXPBY / ZERO on one layout pair; a plan built for
    another kind is never served (the result is asserted at every step), and coming back to a pair
    of values planned before is a hit.  c64 also walks alphas and betas whose real part alone would
    select BITCOPY or ZERO"""
    walk = [(1, 0), (2, 0), (2, 0.5), (0, 0), (0, 1), (1, 0), (2, 0)]
    if ta == CF:
        walk = [(complex(a), complex(b)) for a, b in walk]
        walk += [(1 + 1j, 0), (1j, 0), (1, 1j), (0, 1j), (1, 0), (2 + 1j, 0.5j), (2, 0.5)]
    a_case, c_case = bc_pair("T", 221 + ta, 157)
    v = one(a_case, c_case, "T", ta=ta, tc=tc)
    rig = Rig(gpu, [v])
    seen = set()
    for t, (alpha, beta) in enumerate(walk):
        v.pairs[0].alpha, v.pairs[0].beta = alpha, beta
        d = rig.run(v, t + 1, f"step {t}: alpha {alpha} beta {beta}")
        assert d.hits + d.misses == 1
        if (alpha, beta) in seen:
            assert tuple(d) == HIT, f"step {t}: alpha {alpha} beta {beta} was planned before"
        seen.add((alpha, beta))


# ------------------------------------------------------------------ 3. near misses
def _near_misses():
    """name -> variants that differ in exactly one attribute and share both arenas"""
    n = 157
    out = {}

    def same_bytes(name, m, types, alpha, beta, op="T"):
        a_case, c_case = bc_pair(op, m, n)
        out[name] = [one(a_case, c_case, op, alpha, beta, ta=t, tc=t, name=f"{name}:{t}") for t in types]
    same_bytes("f32-vs-i32", 231, (F, I32), 2, 0)
    same_bytes("f16-vs-bf16", 232, (H16, BF16), 0.75, 0.5)
    same_bytes("e4m3-vs-e5m2", 233, (E4M3, E5M2), 0.5, 2)
    sq = bc_pair("N", 192, 192)
    out["trans-N-vs-T"] = [one(*sq, op, 0.75, -1.5, ta=D, name=f"trans {op}") for op in "NT"]
    sq = bc_pair("T", 176, 176)
    out["trans-T-vs-C"] = [one(*sq, op, 0.75 - 0.5j, 1.25 + 0.25j, ta=CD, name=f"trans {op}") for op in "TC"]
    tri = bc_pair("T", 234, n)
    out["tri-uplo-k"] = [one(*tri, "T", 0.75, -1.5, ta=D, entry="tri", uplo=u, k=k, name=f"tri {u} {k}")
                         for u, k in (("U", 3), ("L", 3), ("U", 4), ("U", 2), ("U", -3))]
    ka = bc_pair("T", 235, n)
    out["ordinary-vs-keep-all-tri"] = [one(*ka, "T", 2, 0.5, ta=D, name="ordinary"),
                                       one(*ka, "T", 2, 0.5, ta=D, entry="tri", uplo="U", k=-10000, name="tri keep-all")]
    out["ordering-C-vs-R"] = [one(*bc_pair("T", 236, n, c_kw=dict(ord=o)), "T", 0.75, -1.5, ta=D, name=f"C ordering {o}")
                              for o in "CR"]
    out["lld-vs-lld+1"] = [one(*bc_pair("T", 237, n, c_kw=dict(lld_pad=p)), "T", 0.75, -1.5, ta=D, name=f"C lld +{p}")
                           for p in (0, 1)]
    out["A-lld-vs-lld+1"] = [one(*bc_pair("T", 238, n, a_kw=dict(lld_pad=p)), "T", 0.75, -1.5, ta=F, name=f"A lld +{p}")
                             for p in (0, 1)]

    def sub(m, ia, ja, subm, subn):  # sub(C) of a (m + 2) x (n + 2) matrix, A whole
        from casegen import BC
        return BC(subn, subm, 32, 48), BC(m + 2, n + 2, 40, 24, ia=ia, ja=ja, subm=subm, subn=subn)
    out["ia-ja-shifted"] = [one(*sub(239, ia, ja, 239, n), "T", 0.75, -1.5, ta=D, name=f"ia {ia} ja {ja}")
                            for ia, ja in ((1, 1), (2, 1), (1, 2))]
    out["subm-smaller"] = [one(*sub(240, 1, 1, sm, sn), "T", 0.75, -1.5, ta=D, name=f"sub {sm} x {sn}")
                           for sm, sn in ((240, n), (239, n), (240, n - 1))]
    out["C-block-size"] = [one(*bc_pair("T", 241, n, c_blk=b), "T", 0.75, -1.5, ta=D, name=f"C blocks {b}")
                           for b in ((40, 24), (40, 25), (41, 24))]
    a_case, c_case = bc_pair("N", 242, n)
    out["A-and-C-swapped"] = [one(a_case, c_case, "N", 0.75, -1.5, ta=D, name="A -> C"),
                              one(c_case, a_case, "N", 0.75, -1.5, ta=D, swapped=True, name="C -> A")]
    a0, c0 = bc_pair("T", 243, n)
    a1, c1 = bc_pair("N", 244, 131, (24, 40), (16, 56))
    ra, rc = (buf_bytes(a0, D) + 511) // 256 * 256, (buf_bytes(c0, D) + 511) // 256 * 256
    p0, p1 = Pair(a0, c0, "T", 2, 0.5), Pair(a1, c1, "N", 3, -1.25, ra, rc)
    out["batch-order"] = [Variant([p0, p1], ta=D, entry="batch", name="[p0, p1]"),
                          Variant([p1, p0], ta=D, entry="batch", name="[p1, p0]"),
                          Variant([p0], ta=D, entry="batch", name="[p0]"),
                          Variant([p1], ta=D, entry="batch", name="[p1]")]
    sw = dict(rowsplit=[0, 37, 77, 117, 150], colsplit=[0, 29, 59, 89, 131])
    zo = np.zeros((4, 4), np.int32)
    src = Moved([0, 50, 131], [0, 70, 150], np.zeros((2, 2), np.int32), gap=1)
    out["custom-C-blocks-swapped"] = [
        one(src, Moved(sw["rowsplit"], sw["colsplit"], zo, gap=1, swap=s), "T", 0.75, -1.5, ta=D, name=f"C swap {s}")
        for s in ((), (5, 9), (6, 10))]
    srcs = [Moved(sw["colsplit"], sw["rowsplit"], zo, gap=1, swap=s) for s in ((), (5, 6))]
    dst = Moved([0, 61, 150], [0, 43, 131], np.zeros((2, 2), np.int32), gap=1)
    out["custom-A-blocks-swapped"] = [one(s, dst, "T", 0.75, -1.5, ta=F, name=f"A swap {s.swap}") for s in srcs]
    return out


NEAR = sorted(_near_misses())
ORDER = {2: [0, 1, 0, 1, 1, 0]}


def _interleave(rig, vs):
    order = ORDER.get(len(vs)) or list(range(len(vs))) + list(range(len(vs)))[::-1] + [1, 0, len(vs) - 1, 0]
    deltas = []
    for t, i in enumerate(order):
        deltas.append((i, rig.run(vs[i], t + 1, f"call {t}: {vs[i].name}")))
    return deltas


@pytest.mark.parametrize("name", NEAR)
def test_near_miss(gpu, name):
    """variants that differ in one attribute, interleaved in the same arenas: every result is its own
    variant's, each variant plans once and replays after that"""
    vs = _near_misses()[name]
    seen = set()
    for i, d in _interleave(Rig(gpu, vs), vs):
        assert tuple(d) == (HIT if i in seen else MISS), f"{vs[i].name}: hits {d.hits} misses {d.misses}"
        seen.add(i)


@pytest.mark.parametrize("residency", ["pageable", "pinned"])
def test_near_miss_host_staging_mode(gpu, residency):
    """host layouts under staging mode 1 and 0, interleaved: each mode has a plan of its own"""
    cases = bc_pair("T", 245 + (residency == "pinned"), 157)
    vs = [one(*cases, "T", 0.75, -1.5, ta=D, host_mode=mode, name=f"staging {mode}") for mode in (1, 0)]
    seen = set()
    for i, d in _interleave(Rig(gpu, vs, residency), vs):
        assert tuple(d) == (HIT if i in seen else MISS), f"{vs[i].name}: hits {d.hits} misses {d.misses}"
        seen.add(i)


# ------------------------------------------------------------------ 4. moved buffers
def _placements(ea, ec):
    """(A shift, C shift) in bytes: every shift on either side, moved independently, in a fixed
    shuffled order, with placements revisited"""
    sa = [0, ea, 16, 16 + ea, 64, 64 + 16, 4096]
    scs = [0, ec, 16, 16 + ec, 64, 64 + 16, 4096]
    pl = [(sa[i], scs[i]) for i in range(7)] + [(sa[i], scs[(3 * i + 2) % 7]) for i in range(7)]
    pl += [(sa[(5 * i + 1) % 7], scs[i]) for i in range(7)]
    rng = np.random.default_rng(0x70C)
    order = list(rng.permutation(len(pl))) + list(rng.permutation(len(pl))[:8])
    return [pl[i] for i in order]


@pytest.mark.parametrize("lld_pad", [0, 1])
@pytest.mark.parametrize("ta,tc,op", [(D, D, "T"), (F, F, "N"), (F, BF16, "T")], ids=["f64-T", "f32-N", "f32-bf16-T"])
def test_moved_buffers(gpu, ta, tc, op, lld_pad):
    """the same geometry with A and C, independently, at byte shifts {0, E, 16, 16 + E, 64, 64 + 16,
    4096} inside the arenas, two calls per placement (new data each), placements in a shuffled fixed
    order and revisited.  Results only, never hit / miss: whatever serves a moved buffer (a new plan
    today) must compute what a plan made for that address computes; VEC flags, granule cuts and
    destination-block groups depend on the address modulo 16, 64 and 128."""
    m = 251 + 2 * ["T", "N"].index(op) + 4 * (tc != ta) + lld_pad  # (a geometry per case)
    cases = bc_pair(op, m, 157, a_kw=dict(lld_pad=lld_pad), c_kw=dict(lld_pad=lld_pad))
    pl = _placements(ESIZE[ta], ESIZE[tc])
    vs = {}
    for sa, scs in pl:
        if (sa, scs) not in vs:
            vs[sa, scs] = one(*cases, op, 0.75, -1.5, sa, scs, ta=ta, tc=tc, name=f"A +{sa} C +{scs}")
    rig = Rig(gpu, list(vs.values()))
    for t, key in enumerate(pl):
        for call in (0, 1):
            rig.run(vs[key], 2 * t + call + 1)


@pytest.mark.parametrize("ta,op", [(D, "T"), (F, "N")], ids=["f64-T", "f32-N"])
def test_moved_custom_blocks(gpu, ta, op):
    """a custom layout whose blocks move each by a different amount, and then two blocks trade places;
    results only"""
    sw = dict(rowsplit=[0, 37, 77, 117, 150], colsplit=[0, 29, 59, 89, 131])
    zo = np.zeros((4, 4), np.int32)
    shifts = (1, 3, 2, 5, 16, 7, 4)

    def cases(a_kw, c_kw):
        ars, acs = (sw["colsplit"], sw["rowsplit"]) if op == "T" else (sw["rowsplit"], sw["colsplit"])
        return Moved(ars, acs, zo, gap=1, **a_kw), Moved(sw["rowsplit"], sw["colsplit"], zo, gap=1, **c_kw)
    mv = dict(shifts=shifts)
    vs = [one(*cases({}, {}), op, 0.75, -1.5, ta=ta, name="base"),
          one(*cases(mv, {}), op, 0.75, -1.5, ta=ta, name="A blocks moved"),
          one(*cases({}, mv), op, 0.75, -1.5, ta=ta, name="C blocks moved"),
          one(*cases(mv, mv), op, 0.75, -1.5, ta=ta, name="both moved"),
          one(*cases(mv, dict(shifts=shifts, swap=(5, 9))), op, 0.75, -1.5, ta=ta, name="moved, C blocks trade"),
          one(*cases(dict(shifts=shifts, swap=(5, 6)), mv), op, 0.75, -1.5, ta=ta, name="moved, A blocks trade")]
    rig = Rig(gpu, vs)
    for t, i in enumerate([0, 1, 0, 2, 3, 4, 3, 5, 4, 0, 5, 3]):
        for call in (0, 1):
            rig.run(vs[i], 2 * t + call + 1)


# ------------------------------------------------------------------ 5. eviction
def _evict_variants(m, count=17, beta=0.5):
    """`count` small variants: one A, a C region each, alpha of its own"""
    a_case, c_case = bc_pair("T", m, 45, (16, 24), (24, 16))
    step = (buf_bytes(c_case, D) + 511) // 256 * 256
    return [one(a_case, c_case, "T", 1 + t, beta, 0, t * step, ta=D, name=f"variant {t}") for t in range(count)]


def test_eviction_sixteen_plans_fit(gpu):
    """16 variants cycled twice: 16 misses, then 16 hits"""
    gpu.release_caches()
    vs = _evict_variants(67, 16)
    rig = Rig(gpu, vs)
    for cycle, want in ((0, MISS), (1, HIT)):
        for t, v in enumerate(vs):
            assert tuple(rig.run(v, 1 + cycle * 16 + t)) == want, f"cycle {cycle}: {v.name}"


def test_eviction_seventeen_plans_thrash(gpu):
    """17 variants cycled twice through 16 slots: each call evicts the plan the next but 15 needs
    (LRU), so 34 misses, and every result is right"""
    gpu.release_caches()
    vs = _evict_variants(68)
    rig = Rig(gpu, vs)
    for cycle in (0, 1):
        for t, v in enumerate(vs):
            assert tuple(rig.run(v, 1 + cycle * 17 + t)) == MISS, f"cycle {cycle}: {v.name}"


@pytest.mark.parametrize("with_host", [False, True], ids=["device", "one-host-variant"])
def test_eviction_under_asynchronous_calls(gpu, with_host):
    """the 17-cycle with transform_async on one torch stream and no synchronise until the end: plans
    are evicted (their device lists freed) while kernels of earlier calls may still be queued; then
    all 17 C regions are checked.  with_host: variant 8 is host-resident (a blocking transform on
    arenas of its own) in the middle of each cycle."""
    gpu.release_caches()
    vs = _evict_variants(69 + with_host)
    rig = Rig(gpu, vs)
    host_rig = None
    if with_host:
        a_case, c_case = vs[8].pairs[0].a_case, vs[8].pairs[0].c_case
        vs[8] = one(a_case, c_case, "T", 9, 0.5, ta=D, name="variant 8 (host)")
        host_rig = Rig(gpu, [vs[8]], "pageable")
    # every device variant reads the shared A region (the same seeded data) and owns a C region; the
    # expected image is built once all regions hold their initial data
    dev_vs = [v for t, v in enumerate(vs) if not (with_host and t == 8)]
    a_img, c_img = rig.A.fresh(), rig.C.fresh()
    for v in dev_vs:
        rig.fill(v, 7, a_img, c_img)
    exp = c_img.copy()
    for v in dev_vs:
        rig.expect(v, a_img, exp, times=2)
    rig.A.put(a_img)
    rig.C.put(c_img)
    if with_host:
        ha, hc_, hexp, _ = host_rig.images(vs[8], 7, times=2)
        host_rig.A.put(ha)
        host_rig.C.put(hc_)
    st0 = gpu.get_stats()
    s = torch.cuda.Stream()
    for cycle in (0, 1):
        for t, v in enumerate(vs):
            if with_host and t == 8:
                host_rig.call(v)
            else:
                rig.call(v, stream=s)
    d = stats_delta(gpu, st0)
    s.synchronize()
    torch.cuda.synchronize()
    assert (d.hits, d.misses) == (0, 34)
    assert_image(rig.C.get(), exp, rig.C, "the 17 C regions after two asynchronous cycles")
    assert_image(rig.A.get(), a_img, rig.A, "A")
    if with_host:
        assert_image(host_rig.C.get(), hexp, host_rig.C, "the host variant's C")


# ------------------------------------------------------------------ 6. one plan, back-to-back calls
_BIG = {}


def _big():
    """2048^2 f64 'T': integer-valued A, C zero; the expected images, computed once"""
    if not _BIG:
        n = 2048
        a_case, c_case = bc_pair("T", n, n, (256, 256), (128, 512))
        rng = np.random.default_rng(0xB16)
        a = rng.integers(-1000, 1000, a_case.buf_elems(0, 1)).astype(np.float64)
        e5 = np.zeros(c_case.buf_elems(0, 1))
        oracle.transform(D, "T", 5, 0, a_case.geom(1), [a], c_case.geom(1), [e5])
        r1 = rng.integers(1, 5, n).astype(np.float64)
        r2 = rng.integers(1, 5, n).astype(np.float64) * 3  # (same sign: no sum or product is a -0.0)
        es = sc.expected_transform(D, D, "T", 1, 0, a_case, c_case, a, np.zeros(c_case.buf_elems(0, 1)), r1 + r2, None)
        for x in (a, e5, es, r1, r2):
            x.setflags(write=False)
        _BIG.update(a_case=a_case, c_case=c_case, a=a, e5=e5, es=es, r1=r1, r2=r2)
    return _BIG


def _big_rig(gpu):
    b = _big()
    v = one(b["a_case"], b["c_case"], "T", 1, 1, ta=D)
    rig = Rig(gpu, [v])
    a_img, c_img = rig.A.fresh(), rig.C.fresh()
    rig.A.region(a_img, 0, D, b["a"].size)[:] = b["a"]
    rig.C.region(c_img, 0, D, b["e5"].size)[:] = 0
    rig.A.put(a_img)
    rig.C.put(c_img)
    return b, v, rig, c_img


@pytest.mark.parametrize("how", ["one-stream", "two-streams", "no-stream"])
def test_back_to_back_async_calls_share_a_plan(gpu, how):
    """transform_async with alpha = 2, then alpha = 3, beta = 1 on the same layouts with no
    synchronise between: the second call rewrites the plan's device scalars while the first call's
    kernels may still be queued.  (a) one torch stream; (b) two torch streams, the second waiting on
    an event of the first as a correct caller would; (c) no stream, then costa.synchronize.  C must
    be exactly 5 * op(A) (integer-valued data).  A pass does not prove the absence of a race; a
    failure proves one."""
    b, v, rig, c_img = _big_rig(gpu)
    A, C = (x[0] for x in rig.layouts(v))
    st0 = gpu.get_stats()
    if how == "one-stream":
        s = torch.cuda.Stream()
        gpu.transform_async(A, C, rig.comm, "T", 2, 1, stream=s)
        gpu.transform_async(A, C, rig.comm, "T", 3, 1, stream=s)
        s.synchronize()
    elif how == "two-streams":
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        gpu.transform_async(A, C, rig.comm, "T", 2, 1, stream=s1)
        ev = torch.cuda.Event()
        ev.record(s1)
        s2.wait_event(ev)
        gpu.transform_async(A, C, rig.comm, "T", 3, 1, stream=s2)
        s2.synchronize()
        s1.synchronize()
    else:
        gpu.transform_async(A, C, rig.comm, "T", 2, 1)
        gpu.transform_async(A, C, rig.comm, "T", 3, 1)
        gpu.synchronize(rig.comm)
    d = stats_delta(gpu, st0)
    assert d.hits + d.misses == 2 and d.hits >= 1, "the second call replays the first call's plan"
    exp = c_img.copy()
    rig.C.region(exp, 0, D, b["e5"].size)[:] = b["e5"]
    assert_image(rig.C.get(), exp, rig.C, f"C after alpha 2 then 3 ({how})")


@pytest.mark.parametrize("how", ["one-stream", "two-streams"])
def test_back_to_back_scaled_calls_share_a_plan(gpu, how):
    """the same with a scaled plan and two different row_scale vectors (alpha = beta = 1): C must be
    exactly op(A) * (r1 + r2) row by row.  A pass does not prove the absence of a race; a failure
    proves one."""
    b, v, rig, c_img = _big_rig(gpu)
    A, C = (x[0] for x in rig.layouts(v))
    r1, r2 = torch.from_numpy(b["r1"].copy()).cuda(), torch.from_numpy(b["r2"].copy()).cuda()
    torch.cuda.synchronize()
    st0 = gpu.get_stats()
    s1 = torch.cuda.Stream()
    s2 = s1 if how == "one-stream" else torch.cuda.Stream()
    gpu.transform_scaled(A, C, rig.comm, "T", 1, 1, row_scale=r1, stream=s1)
    if s2 is not s1:
        ev = torch.cuda.Event()
        ev.record(s1)
        s2.wait_event(ev)
    gpu.transform_scaled(A, C, rig.comm, "T", 1, 1, row_scale=r2, stream=s2)
    s2.synchronize()
    s1.synchronize()
    d = stats_delta(gpu, st0)
    assert d.hits + d.misses == 2 and d.hits >= 1
    exp = c_img.copy()
    rig.C.region(exp, 0, D, b["es"].size)[:] = b["es"]
    assert_image(rig.C.get(), exp, rig.C, f"C after row_scale r1 then r2 ({how})")


# ------------------------------------------------------------------ 7. lifetime
def test_rebuilt_layouts_hit(gpu):
    """both Layouts closed and rebuilt with identical content: the key is content, not handles"""
    v = one(*bc_pair("T", 261, 157), "T", 0.75, -1.5, ta=D)
    rig = Rig(gpu, [v])
    assert tuple(rig.run(v, 1)) == MISS
    rig.forget(v)
    assert tuple(rig.run(v, 2)) == HIT
    rig.forget(v)
    assert tuple(rig.run(v, 3)) == HIT


def test_release_caches_then_plan_again(gpu):
    """release_caches(): the next call is a miss and right, later calls hit again"""
    v = one(*bc_pair("T", 262, 157), "T", 0.75, -1.5, ta=D)
    rig = Rig(gpu, [v])
    assert tuple(rig.run(v, 1)) == MISS
    assert tuple(rig.run(v, 2)) == HIT
    gpu.release_caches()
    assert tuple(rig.run(v, 3)) == MISS
    assert tuple(rig.run(v, 4)) == HIT
    assert tuple(rig.run(v, 5)) == HIT


def test_planner_mode_is_not_part_of_the_key(gpu):
    """set_planner(2): a first call plans on the GPU (device_plans + 1); after set_planner(1) the same
    call hits that plan and is right.  Then the reverse order: a host-built plan serves the call
    made under set_planner(2).  (Both planners give the same plan.)"""
    v, w = (one(*bc_pair("T", 263 + t, 157), "T", 0.75, -1.5, ta=D) for t in (0, 1))
    rig = Rig(gpu, [v, w])
    try:
        gpu.set_planner(2)
        d = rig.run(v, 1)
        assert (tuple(d), d.device_plans) == (MISS, 1)
        gpu.set_planner(1)
        d = rig.run(v, 2)
        assert (tuple(d), d.device_plans) == (HIT, 0)
        d = rig.run(w, 3)
        assert (tuple(d), d.device_plans) == (MISS, 0)
        gpu.set_planner(2)
        d = rig.run(w, 4)
        assert (tuple(d), d.device_plans) == (HIT, 0)
    finally:
        gpu.set_planner(1)
