"""CPU: the planners' and the work-list builders' 64-bit address arithmetic on buffers past 4 GiB and
2^31 elements, at fake base addresses (nothing is dereferenced).

  * every stretched case of tests/test_gpu_extents.py passes its host checks here too (footprints
    inside the allocation, the threshold crossed by the sub-tiles of the lists that would run);
  * element maps: the ops of the plain, mixed, tri and scaled exports of stretched layout pairs,
    expanded to (destination address -> source address) with numpy int64, equal the closed form
    computed from the layout parameters alone, every element of sub(C) exactly once;
  * the work lists of a stretched op list equal its twin's except for addresses and leading
    dimensions, wherever the builder does not branch on size; the branches are named;
  * `work_check extents` (tools/work_check.cpp): element-exact coverage of stretched plain and strip
    lists, the granule_split bail-out and the panel key's address-order fallback;
  * the limits are refusals (COSTA_ERR_ARG), and transform_tri's k at +-2^30 and +-(2^31 - 1).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import stretch_common as sc
from casegen import BC
from tri_common import kept_of_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "costa_amd", "lib")
A0, C0 = 1 << 40, 1 << 44  # fake bases, 16 TiB apart


def _ids(specs):
    return [pytest.param(s, id=s.id) for s in specs]


ALL = sc.plain_specs() + sc.custom_specs() + sc.strip_specs() + sc.mx_specs()


@pytest.mark.parametrize("s", _ids(ALL))
def test_host_checks_of_every_gpu_case(costa, s):
    a_big, c_big = s.big()
    assert sc.big_bytes(a_big, s.ta) <= sc.SIDE_LIMIT and sc.big_bytes(c_big, s.tc) <= sc.SIDE_LIMIT
    assert sc.big_bytes(a_big, s.ta) + sc.big_bytes(c_big, s.tc) <= sc.TEST_LIMIT - sc.GIB
    for case in (a_big, c_big):
        if case is not s.a_twin and case is not s.c_twin:
            with pytest.raises(AssertionError, match="never reach the host"):
                case.buf_elems(0, 1)
    sc.host_checks(costa, s, a_big, c_big, A0, C0)


def test_subtile_exports_of_the_mx_and_block_scaled_pairs(costa):
    """the grids assertion (b) is made on come from the library (costa_hip_mx_subtile / _block_subtile):
    every pair of the stretched cases has one, a pair that does not exist is refused"""
    for s in sc.mx_specs():
        bf, bs = (costa.block_subtile if s.family == "bs" else costa.mx_subtile)(s.ta, s.tc)
        assert bf > 0 and bs > 0
    assert costa.block_subtile(0, 8) >= costa.block_subtile(8, 0)  # (a quantising pair runs whole regions)
    for fn, pair in ((costa.mx_subtile, (1, 1)), (costa.block_subtile, (0, 0)), (costa.block_subtile, (9, 0))):
        with pytest.raises(costa.CostaError) as e:
            fn(*pair)
        assert e.value.code == 1


def test_stretching_keeps_the_alignment_class():
    """+ k * 256 elements: ld * E mod 64 bytes is kept for every element size, FP4 and FP6 included"""
    for code, qb in sc.QB.items():
        for lld in (300, 301, 304, 262):
            if (lld * qb) % 4:
                continue
            big = sc.stretched(BC(lld, 40, lld, 40), sc.threshold_elems("bytes", code))
            assert (big.sizes(1)[0] * qb // 4) % 64 == (lld * qb // 4) % 64


# ------------------------------------------------------------------ element maps
def _pairs():
    """stretched block-cyclic pairs: 'N' / 'T', orderings C and R, sub-matrix offsets, aligned and odd
    pads, blocks that do not match; and the two-arena custom pair"""
    out = []
    m, n = 230, 310
    for op in ("N", "T"):
        am, an = (n, m) if op == "T" else (m, n)
        out.append((f"bc-{op}-aligned", op, BC(am, an, 24, 24), BC(m, n, 40, 56)))
        out.append((f"bc-{op}-odd-rowmajor", op, BC(am, an, 32, 48, ord="R", lld_pad=1), BC(m, n, 40, 24, lld_pad=3)))
        # one block on one side cut by the other side's grid: sub_tile()'s offset inside a block is
        # the large number here (with small blocks on both sides it is the layouts' block addresses)
        out.append((f"bc-{op}-oneblock-A", op, BC(am, an, am, an, lld_pad=1), BC(m, n, 40, 24)))
        out.append((f"bc-{op}-oneblock-C", op, BC(am, an, 32, 48), BC(m, n, m, n, ord="R")))
        out.append((f"bc-{op}-sub", op, BC(am + 20, an + 30, 24, 24, ia=9, ja=17, subm=am, subn=an, lld_pad=2),
                    BC(m + 13, n + 5, 64, 64, ia=4, ja=2, subm=m, subn=n, ord="R")))
    for s in sc.custom_specs()[::2]:
        out.append((f"arenas-{s.op}", s.op, s.a_twin, s.c_twin))
    return out


def _stretch(case, code):
    if isinstance(case, BC):  # (both rules at once where the type has an element rule)
        thr = sc.threshold_elems("bytes", code)
        return sc.stretched(case, max(thr, sc.ELEM_RULE) if sc.QB[code] <= 16 else thr)
    return sc.TwoArena(case, sc.threshold_elems("bytes", code) + sc.STEP)


def _closed_form(a_big, c_big, ta, tc, op):
    m, n = c_big.shape()
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(m, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij"))
    dst = sc.element_address(c_big, C0, tc, i, j)
    src = sc.element_address(a_big, A0, ta, j, i) if op != "N" else sc.element_address(a_big, A0, ta, i, j)
    assert dst.max() - C0 >= sc.BYTE_RULE and src.max() - A0 >= sc.BYTE_RULE  # (the pair is stretched)
    return i, j, dst, src


def _assert_map(dst, src, want_dst, want_src, what):
    o, w = np.argsort(dst, kind="stable"), np.argsort(want_dst, kind="stable")
    assert dst.size == want_dst.size, f"{what}: {dst.size} elements moved, sub(C) has {want_dst.size}"
    assert np.unique(dst).size == dst.size, f"{what}: an element of C is written twice"
    assert np.array_equal(dst[o], want_dst[w]), f"{what}: the destination addresses are not sub(C)'s"
    bad = np.flatnonzero(src[o] != want_src[w])
    assert bad.size == 0, (f"{what}: {bad.size} elements come from the wrong source address, first C address "
                           f"{int(dst[o][bad[0]]):#x}: {int(src[o][bad[0]]):#x}, expected {int(want_src[w][bad[0]]):#x}")


@pytest.mark.parametrize("kind", ["plain", "mixed", "tri", "scaled"])
@pytest.mark.parametrize("name,op,a_twin,c_twin", _pairs(), ids=[p[0] for p in _pairs()])
def test_element_map_of_stretched_pairs(costa, kind, name, op, a_twin, c_twin):
    ta, tc = {"plain": (1, 1), "mixed": (1, 0), "tri": (0, 0), "scaled": (6, 0)}[kind]
    a_big, c_big = _stretch(a_twin, ta), _stretch(c_twin, tc)
    LA, LC = sc.make_layout(costa, a_big, A0, ta), sc.make_layout(costa, c_big, C0, tc)
    i, j, want_dst, want_src = _closed_form(a_big, c_big, ta, tc, op)
    what = f"{kind} {name}"
    if kind in ("plain", "mixed"):
        p = costa.plan_export([LA], [LC], 0, 1, [op], [-0.5], [2.0])
        dst, src, *_ = sc.expand_ops(p.local_ops, ta, tc)
    elif kind == "scaled":
        p = costa.plan_export_scaled(LA, LC, 0, 1, op, -0.5, 2.0)
        ops = p.local_scaled
        dst, src, x, f, s = sc.expand_ops(ops, ta, tc)
        # ... and each op's (row0, col0, F_ROWS) name the target position of its elements
        frow = (ops["op"]["flags"][x] & 0x80) != 0
        ti = ops["row0"][x].astype(np.int64) + np.where(frow, f, s)
        tj = ops["col0"][x].astype(np.int64) + np.where(frow, s, f)
        assert np.array_equal(sc.element_address(c_big, C0, tc, ti, tj), dst), f"{what}: row0 / col0 / F_ROWS"
    else:
        m, n = c_big.shape()
        uplo, k = ("U", -7) if op == "N" else ("L", 11)
        p = costa.plan_export_tri(LA, LC, 0, 1, op, uplo, k, -0.5, 2.0)
        d1, s1, *_ = sc.expand_ops(p.local_ops, ta, tc)
        d2, s2, *_ = sc.expand_ops(p.local_tri, ta, tc, keep=lambda t: kept_of_op(t)[1])
        dst, src = np.concatenate([d1, d2]), np.concatenate([s1, s2])
        keep = (j - i >= k) if uplo == "U" else (j - i <= k)
        assert 0 < keep.sum() < keep.size and p.local_tri.size > 0
        want_dst, want_src = want_dst[keep], want_src[keep]
    assert p.pack_ops.size == 0
    _assert_map(dst, src, want_dst, want_src, what)


# ------------------------------------------------------------------ stretched lists against their twins
def _cols(ops):
    """op records without addresses and leading dimensions"""
    return np.stack([ops[k].astype(np.int64) for k in ("nf", "ns", "flags", "order")]).tobytes()


def _normal(w):
    """a work list without addresses and leading dimensions (a group's header keeps its op count in
    `src`; the staged image's size follows the pitch)"""
    return _cols(w.ordered), w.work.tobytes(), {k: v for k, v in w.meta.items() if k not in ("on_gpu", "cblock_lds")}


def _classes(w):
    return tuple(int(w.meta[k]) for k in ("n_large", "n_medium", "n_skew", "n_cblock", "n_tiny"))


def _branch(code, t_ops, t, b_ops, b):
    """What the twin's lists (t) and the stretched lists (b) SHOW -> None when they are the same lists
    but for addresses and leading dimensions, else the size-dependent branch of build_work (engine.cpp)
    that explains the difference; the branch's own condition on the ops must hold, anything else fails.
      groups        the twin forms destination-block groups, the stretched list none: an op may join a
                    group only while ldd <= the group budget
      address-order the same records in another order where the ops' destination addresses are in
                    another order (the two arenas): groups and pieces are listed by destination address
      group-budget  the same rule seen without a group: transposes into a pitch within the budget stay
                    on the wavefront path for the groups to find (pieces), past it they take the skew shape
    (The panel walk of address-sorted sub-tiles, ldd * E > 128 KiB, cannot tell a twin from its stretched
    list: a matrix whose twin has no panels has at most 128 KiB of rows, one panel, and one panel's order
    is the plain address order.  `work_check cover` and `work_check extents` pin it.)"""
    import tile_lists
    if _normal(t) == _normal(b):
        return None
    E = sc.QB[code] // 4
    budget = tile_lists.group_budget(E)
    ct, cb = _classes(t), _classes(b)
    tl, bl = t_ops["ldd"].astype(np.int64), b_ops["ldd"].astype(np.int64)
    within = code in (0, 1, 4) and (tl <= budget).all() and (bl > budget).all()
    rows = lambda w: np.sort(np.stack([w.ordered[k].astype(np.int64) for k in ("nf", "ns", "flags", "order")], 1), 0)
    if ct == cb and np.array_equal(rows(t), rows(b)):
        assert not np.array_equal(np.argsort(t_ops["dst"], kind="stable"), np.argsort(b_ops["dst"], kind="stable")), \
            "the same destination order, yet the records are listed in another"
        return "address-order"
    if ct[3] > 0 and cb[3] == 0:
        assert within, "groups vanished where the group budget does not explain it"
        return "groups"
    if ct[3] == cb[3] == 0 and ct[2] == 0 and ct[4] > 0 and cb[2] > 0:
        assert within and ((b_ops["flags"] & 1) != 0).all(), "pieces became skew items where the budget does not explain it"
        return "group-budget"
    raise AssertionError(f"the lists differ and no size-dependent branch explains it: classes {ct} against {cb}")


def _grouped_pairs():
    """a ragged custom pair whose target blocks have their own compact pitch (groups form), against
    the same pair with 8192 elements of padding in every target column (past the group budget)"""
    from casegen import Custom
    out = []
    for s in sc.custom_specs()[::2]:
        c = s.c_twin
        wide = Custom(c.rowsplit, c.colsplit, c.owners, ord=c.ord, ld_pad=8192, gap=c.gap)
        out.append(pytest.param(s, s.a_twin, wide, id=f"custom-{s.op}-compact-vs-wide"))
    return out


def _twin_and_big(costa, s, a_big, c_big):
    out = []
    for a, c in ((s.a_twin, s.c_twin), (a_big, c_big)):
        LA, LC = sc.make_layout(costa, a, A0, s.ta), sc.make_layout(costa, c, C0, s.tc)
        p = costa.plan_export([LA], [LC], 0, 1, [s.op], [s.alpha], [s.beta])
        out += [p.local_ops, costa.work_export(s.ta, p.local_ops)]
    return out


def _panel_pair():
    """fp64 'T' into an aligned pitch of 2048 (past the group budget, a 16 KiB column): the stretched
    list's address-sorted sub-tiles take the panel key, with one panel; the lists must be the same"""
    s = sc.Spec("plain", 1, 1, "T", 1.0, 0.0, BC(160, 2048, 128, 128), BC(2048, 160, 128, 128), tag="panels")
    return [pytest.param(s, *s.big(), id=s.id)]


_LIST_CASES = ([pytest.param(s, *s.big(), id=s.id) for s in sc.plain_specs() + sc.custom_specs()] + _grouped_pairs()
               + _panel_pair())
_SEEN = {}


@pytest.mark.parametrize("s,a_big,c_big", _LIST_CASES)
def test_stretched_lists_equal_their_twins(costa, s, a_big, c_big, request):
    t_ops, t, b_ops, b = _twin_and_big(costa, s, a_big, c_big)
    # the planners never branch on a size: the op lists differ in addresses and leading dimensions only
    assert _cols(t_ops) == _cols(b_ops)
    branch = _branch(s.ta, t_ops, t, b_ops, b)  # (None: the strict comparison held)
    _SEEN[request.node.callspec.id] = branch
    if s.family == "custom" and isinstance(a_big, sc.TwoArena):
        # groups and pieces on both sides, the same ones
        assert branch == "address-order" and _classes(t) == _classes(b) and _classes(t)[3] > 0 and _classes(t)[4] > 0
    if branch is not None:  # the same elements either way, listed differently
        area = lambda ops: int((sc.plain_lists(costa, s.ta, ops)[2]["nf"].astype(np.int64)
                                * sc.plain_lists(costa, s.ta, ops)[2]["ns"]).sum())
        assert area(t_ops) == area(b_ops) == int((t_ops["nf"].astype(np.int64) * t_ops["ns"]).sum())


def test_every_size_branch_is_met(costa):
    """each named branch is taken by the lists of some case above (not merely allowed by its sizes), the
    strict comparison holds for copies and transposes of real and complex types, and a twin really
    forms groups that its stretched list does not.  (granule_split's bail-out and the panel key's
    fallback need pitches of 33.5 M and 2^30 elements: `work_check extents`.)"""
    seen = {}
    for prm in _LIST_CASES:
        s, a_big, c_big = prm.values
        t_ops, t, b_ops, b = _twin_and_big(costa, s, a_big, c_big)
        seen.setdefault(_branch(s.ta, t_ops, t, b_ops, b), []).append((s, _classes(t), _classes(b)))
    assert {None, "groups", "group-budget", "address-order"} == set(seen), set(seen)
    assert all(ct[3] > 0 and cb[3] == 0 for _, ct, cb in seen["groups"])
    strict = {(s.ta, s.op) for s, _, _ in seen[None]}
    assert any(s.tag == "panels" for s, _, _ in seen[None])
    assert {(0, "N"), (1, "N"), (4, "N"), (2, "N"), (3, "N"), (2, "C"), (3, "C")} <= strict, strict


# ------------------------------------------------------------------ work_check extents
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_work_check_extents(tmp_path):
    if not os.path.exists(os.path.join(LIB, "libcosta_amd.so")):
        pytest.skip("libcosta_amd.so not built (run __graft_entry__.build())")
    exe = tmp_path / "work_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "costa_amd", "csrc"),
                    os.path.join(ROOT, "tools", "work_check.cpp"), "-L" + LIB, "-lcosta_amd",
                    "-Wl,-rpath," + LIB, "-o", str(exe)], check=True, timeout=300)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("COSTA_")}
    r = subprocess.run([str(exe), "extents"], capture_output=True, text=True, timeout=300, env=clean)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    for line in ("granule bail-out: pitch 33554433 left whole", "panel key fallback: ldd 1073741824 plain address order",
                 "strip and plain limits: 7 of 7 refused"):
        assert line in r.stdout, r.stdout
    # destination-block groups with wavefront pieces, and a medium class of 4096 ops or more, were walked
    import re
    g = [int(x) for x in re.findall(r"extents groups .*? (\d+) groups, \d+ pieces", r.stdout)]
    assert len(g) == 2 and min(g) > 0, r.stdout
    assert re.search(r"extents medium .* 4160 medium", r.stdout), r.stdout


# ------------------------------------------------------------------ limits
def _op(costa, nf, ns, lds, ldd, flags=0x20):
    ops = np.zeros(1, costa.TILE_OP_DTYPE)
    ops[0] = (A0, C0, nf, ns, lds, ldd, flags, 1)
    return ops


def test_limits_are_refusals(costa):
    """hand-made ops, nothing allocated: an op of more sub-tiles than a work item can name is refused
    with COSTA_ERR_ARG before anything is built or launched; one just below the limit is listed"""
    big = 2 ** 31 - 1
    # (a copy of this size used to look tiny: is_tiny()'s nf * ns * E passed 2^63)
    for code, flags in ((1, 0x20), (1, 0x2c), (1, 0x21), (3, 0x21), (0, 0x2d)):
        with pytest.raises(costa.CostaError, match="tile too large") as e:
            costa.work_export(code, _op(costa, big, big, big, big, flags))
        assert e.value.code == 1
    # ... and far from INT32_MAX: 2^28 x 2^28 is 2^21 x 2^24 sub-tiles of 128 x 16
    for flags in (0x2c, 0x2d, 0x20):
        with pytest.raises(costa.CostaError, match="tile too large") as e:
            costa.work_export(1, _op(costa, 1 << 28, 1 << 28, 1 << 28, 1 << 28, flags))
        assert e.value.code == 1
    # f64 copies: 128 x 16 sub-tiles; 2^24 x 2^15 of them = 2^32 - ... stay below
    w = costa.work_export(1, _op(costa, 1 << 20, 1 << 12, 1 << 20, 1 << 20))
    assert w.meta["n_large"] == (1 << 13) * (1 << 8)
    # (the strip builders' "list too long": `work_check extents`, they have no export)


@pytest.mark.parametrize("uplo", ["U", "L"])
@pytest.mark.parametrize("k", [2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, -(2 ** 30 - 1), -(2 ** 30), -(2 ** 30 + 1),
                               -(2 ** 31 - 1)])
@pytest.mark.parametrize("op", ["N", "T"])
def test_tri_plans_at_extreme_k(costa, op, uplo, k):
    """the diagonal is clamped at +-2^30 in tri_op(): far outside a 70 x 50 matrix either way, so the
    plan keeps everything or nothing, as numpy.triu / tril do"""
    m, n = 70, 50
    am, an = (n, m) if op == "T" else (m, n)
    a, c = BC(am, an, 32, 16), BC(m, n, 24, 40, lld_pad=1)
    LA, LC = a.make_layout(0, A0, 1, 1), c.make_layout(0, C0, 1, 1)
    p = costa.plan_export_tri(LA, LC, 0, 1, op, uplo, k, 1.0, 0.0)
    ref = (np.triu if uplo == "U" else np.tril)(np.ones((m, n)), k)
    assert ref.sum() in (0, m * n)
    d1, *_ = sc.expand_ops(p.local_ops, 1, 1)
    d2, *_ = sc.expand_ops(p.local_tri, 1, 1, keep=lambda t: kept_of_op(t)[1])
    assert d1.size + d2.size == int(ref.sum()) and np.unique(np.concatenate([d1, d2])).size == int(ref.sum())
