"""Census of the tile kernels' launch variants on the CPU: every launch tile_kernels.hip launch_t can
issue for a type is pinned by a list of tests/tile_lists.py that declares it, and every list's
declaration holds under the default dispatch (engine.cpp build_work through
costa_hip_work_export's host builder; no kernel runs).  tests/test_gpu_tiles.py runs the same lists
bit-exact against the oracle."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.path.exists(os.path.join(ROOT, "costa_amd", "lib", "libcosta_amd.so")):
    pytest.skip("libcosta_amd.so not built (run __graft_entry__.build())", allow_module_level=True)

import oracle  # noqa: E402
import tile_lists  # noqa: E402

# tile_kernels.hip launch_cblock (real types only) x launch_cblock_v<T, TR, AX>, alone or with the
# wavefront pieces fused (launch_t: pieces_in_group_launch)
_GROUPS = {f"cblock_{s}{p}" for s in ("N", "T", "Nax", "Tax") for p in ("", "+pieces")}
# tile_kernels.hip launch_tiny: launch_tiny_v<T, W, TR, AX>, every type
_TINY = {f"tiny_{s}" for s in ("N", "T", "Nax", "Tax")}

# what exists per type, by hand from tile_kernels.hip
REACHABLE = {
    "f32": {"large",             # shapes<float>::large
            "large_tr",          # shapes<float>::large_tr (large_tr_full and small_tr alias it; has_small = false)
            "medium_tr",         # shapes<float>::medium_tr, has_medium = true
            "medium_tr_full",    # shapes<float>::medium_tr_full: shape<float, 128, 64, 64>, a kernel of its own
            "small32_tr",        # shapes<float>::small32_tr
            "skew",              # launch_skew: float, skew_kernel<T, false>
            "skew_wide",         # launch_skew: sizeof(T) == 4, skew_kernel<T, true>
            } | _GROUPS | _TINY,
    "i32": {"large",             # shapes<int>::large
            "large_tr",          # shapes<int>::large_tr (large_tr_full and small_tr alias it; has_small = false)
            "medium_tr",         # shapes<int>::medium_tr, has_medium = true
            "medium_tr_full",    # shapes<int>::medium_tr_full: shape<int, 128, 64, 64>, a kernel of its own
            "small32_tr",        # shapes<int>::small32_tr
            "skew",              # launch_skew: int, skew_kernel<T, false>
            "skew_wide",         # launch_skew: sizeof(T) == 4, skew_kernel<T, true>
            } | _GROUPS | _TINY,
    "f64": {"large",             # shapes<double>::large
            "large_tr",          # shapes<double>::large_tr (large_tr_full aliases it)
            "small_tr",          # shapes<double>::small_tr: shape<double, 512, 64, 64>, has_small = true
            "medium_tr",         # shapes<double>::medium_tr, has_medium = true (medium_tr_full aliases it)
            "small32_tr",        # shapes<double>::small32_tr
            "skew",              # launch_skew: double, skew_kernel<T, false> (no wide variant: 8 bytes)
            } | _GROUPS | _TINY,
    "c64": {"large",             # shapes<cpx<float>>::large
            "large_tr",          # shapes<cpx<float>>::large_tr (large_tr_full aliases it; has_medium = false)
            "small_tr",          # shapes<cpx<float>>::small_tr: shape<cpx<float>, 512, 64, 64>
            "small32_tr",        # shapes<cpx<float>>::small32_tr
            } | _TINY,           # (launch_skew and launch_cblock throw for complex types)
    "c128": {"large",            # shapes<cpx<double>>::large
             "large_tr",         # shapes<cpx<double>>::large_tr: 1024 threads (has_medium = false)
             "large_tr_full",    # shapes<cpx<double>>::large_tr_full: shape<cpx<double>, 256, 64, 128>, its own kernel
             "small_tr",         # shapes<cpx<double>>::small_tr: shape<cpx<double>, 1024, 64, 64>
             "small32_tr",       # shapes<cpx<double>>::small32_tr
             } | _TINY,
}
# type -> {variant: the build_work reasoning why no list reaches it under the default knobs}
UNREACHABLE = {t: {} for t in REACHABLE}


def _declared_by_type():
    got = {t: {} for t in REACHABLE}
    for name, (code, _, declared) in tile_lists.LISTS.items():
        for v in declared:
            got[tile_lists.NAMES[code]].setdefault(v, []).append(name)
    return got


@pytest.mark.parametrize("name", list(tile_lists.LISTS))
def test_list_takes_its_route(name):
    """declared <= variants() and the split fields the list pins; its ops stay inside its buffers"""
    code, ops, n_src, n_dst = tile_lists.extents(name)
    assert tile_lists.LISTS[name][2], f"{name} declares no launch"
    tile_lists.check_route(name, ops)
    E = np.dtype(oracle.NP[code]).itemsize
    nf, ns, lds, ldd = (ops[k].astype(np.int64) for k in ("nf", "ns", "lds", "ldd"))
    tr = (ops["flags"] & 1).astype(bool)
    run, runs = np.where(tr, ns, nf), np.where(tr, nf, ns)
    assert (ops["src"] % E == 0).all() and (ops["dst"] % E == 0).all()
    assert (lds >= nf).all() and (ldd >= run).all()
    assert ((ops["src"] // E).astype(np.int64) + (ns - 1) * lds + nf <= n_src).all()
    assert ((ops["dst"] // E).astype(np.int64) + (runs - 1) * ldd + run <= n_dst).all()


def test_every_variant_has_a_list():
    """per type, the union of the declarations is exactly what exists: a cell without a list, or a
    declaration of something the type does not have, names itself"""
    got = _declared_by_type()
    for t, want in REACHABLE.items():
        missing = want - set(got[t]) - set(UNREACHABLE[t])
        extra = set(got[t]) - want
        assert not missing, f"{t}: no registry list declares {sorted(missing)}"
        assert not extra, f"{t}: lists declare {sorted(extra)}, which tile_kernels.hip does not have for it"
        assert not set(UNREACHABLE[t]) & set(got[t]), f"{t}: listed unreachable but declared"


def test_variant_names_are_accounted_for():
    """every name variants() can return is reachable or excused, and nothing else is in the tables"""
    for t in REACHABLE:
        assert tile_lists.possible(t) == REACHABLE[t] | set(UNREACHABLE[t]), t


def test_every_list_has_a_gpu_test():
    """the registry and tests/test_gpu_tiles.py agree: each prefix has a test there, parametrised
    over exactly the registry's lists of that prefix"""
    pytest.importorskip("torch")
    import test_gpu_tiles
    prefixes = {name.split("[")[0] for name in tile_lists.LISTS}
    assert prefixes == set(test_gpu_tiles.TESTS), prefixes ^ set(test_gpu_tiles.TESTS)
    for prefix, fn in test_gpu_tiles.TESTS.items():
        marks = [m for m in getattr(getattr(test_gpu_tiles, fn), "pytestmark", []) if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].args[0] == "name", f"{fn}: not parametrised over the registry"
        want = [n for n in tile_lists.LISTS if n.startswith(prefix + "[")]
        assert list(marks[0].args[1]) == want, f"{fn} runs {marks[0].args[1]}, the registry has {want}"


# cells whose launch can only run whole sub-tiles under the default knobs, with the reason
WHOLE_ONLY = {
    # engine.cpp build_work: with the square shape on, fp64's large class starts at q_lo = sub_elems
    # (a medium tier exists) = 64 * 128 / 2 = 4096 elements, and sq needs nf <= 64 and ns <= 64: only
    # exact 64 x 64 ops; an unaligned one leaves the class (wave policy 2: !aligned && elems <=
    # kUnalignedWaveCap * sub_elems)
    ("f64", "small_tr"),
}


def test_sub_tile_mix():
    """per type and shaped launch, the lists that declare it hold whole sub-tiles (run_tile's FULL
    instantiation) and guarded ones (ragged edge or unaligned), counted from the executor's own work
    items; transposing shapes also both kinds among transposing ops.  *_full launches and the
    WHOLE_ONLY cells: whole ones only"""
    total = {}
    for name, (code, _, declared) in tile_lists.LISTS.items():
        if not declared & set(tile_lists.SHAPED):
            continue
        ops = tile_lists.ops_of(name)[1]
        for v, c in tile_lists.subtiles(code, ops).items():
            if v in declared:
                acc = total.setdefault((tile_lists.NAMES[code], v), dict.fromkeys(c, 0))
                for k in c:
                    acc[k] += c[k]
    cells = {(t, v) for t in REACHABLE for v in REACHABLE[t] if v in tile_lists.SHAPED}
    assert set(total) == cells, set(total) ^ cells
    for (t, v), c in sorted(total.items()):
        print(t, v, c)
        if v.endswith("_full") or (t, v) in WHOLE_ONLY:
            assert c["whole"] > 0 and c["whole_tr"] > 0 and c["guarded"] == 0, f"{t} {v}: {c}"
            continue
        assert c["whole"] > 0 and c["guarded"] > 0, f"{t} {v}: one path of run_tile never runs: {c}"
        if v != "large":
            assert c["whole_tr"] > 0 and c["guarded_tr"] > 0, f"{t} {v}: among transposing ops: {c}"


# ---------------------------------------------------------------------------- special values
# sha256 over (ops, source, initial destination, scalars) of build(name) without specials: the
# special-value modes must leave the default data of every list as it was
_DEFAULT_SHA = {
    "mixed[2-c64]": "fc07be6bc8a1091dc7fbeb0dd0c8c08afaace6d96d1c57ae1ea3ae4d2781f945",
    "medium[f64-mix]": "cbb084a120f2993a952d0ed6a9743d034bc90fc4739af9986188f783dd87be5d",
    "square[1-c128]": "de445e583d150167aa7c7c2bb22db6ee5d459361a203ecde7c07399ccf6cd90f",
    "full[c128]": "c913a854b7bd97864b56ab2d9c7b2ddfeb2f55e25170d98aa52b721ac1d92c1c",
    "group[Tax+p-f32]": "1e271c7cd5b6a9acc8ee25da5496d57160ddc2abeeb79206e2027d9898df8f6a",
    "skew[off16-f64]": "b689934124acb177b4b95460982e1177bb963c046133f9221a4672b58f831d45",
}


@pytest.mark.parametrize("name", list(_DEFAULT_SHA))
def test_default_list_data_is_unchanged(name):
    import hashlib
    _, ops, src, dst0, scal, _ = tile_lists.build(name)
    h = hashlib.sha256()
    for a in (ops, src, dst0, scal):
        h.update(a.tobytes())
    assert h.hexdigest() == _DEFAULT_SHA[name]
    # and the special-value modes change the data, not the ops
    _, ops2, src2, dst2, scal2, _ = tile_lists.build(name, "huge")
    assert ops2.tobytes() == ops.tobytes() and scal2[:4].tobytes() == scal[:4].tobytes()
    assert src2.tobytes() != src.tobytes() and dst2.tobytes() != dst0.tobytes() and scal2[7] != scal[7]


def test_real_special_value_lists_cover_every_launch():
    """test_gpu_tiles.REAL_SPECIALS names, per real floating type, one list for every launch the
    type has, and each list declares that launch"""
    pytest.importorskip("torch")
    import test_gpu_tiles
    for t, table in test_gpu_tiles.REAL_SPECIALS.items():
        assert set(table) == REACHABLE[t], f"{t}: {sorted(set(table) ^ REACHABLE[t])}"
        for v, name in table.items():
            code, _, declared = tile_lists.LISTS[name]
            assert tile_lists.NAMES[code] == t and v in declared, f"{name} does not declare {t} {v}"
    want = [(n, m) for n, (c, _, _) in tile_lists.LISTS.items() if tile_lists.NAMES[c] in ("c64", "c128")
            for m in _MODES]
    assert test_gpu_tiles.SPECIAL_CASES[:len(want)] == want, "every complex list runs in both modes"


_MODES = ("drawn", "huge")
# the ops a shaped launch runs, where not both kinds: `large` is the copy shape (lists without a
# transposing op), and the lists of the 32 x 32 shape hold transposing ops only (medium_list)
_OP_MODES = {"large": ("copy",), "small32_tr": ("tr",)}
# launches whose lists hold no conjugating op (medium_list draws none)
_NO_CONJ = {"small32_tr"}
# (type, launch) that cannot run a guarded sub-tile, with the reason (as WHOLE_ONLY above)
_REDO_WHOLE_ONLY = {
    # engine.cpp work_split::full: the launch is chosen only when every sub-tile of the list is whole
    ("c128", "large_tr_full"),
}


@pytest.mark.parametrize("t", ["c64", "c128"])
def test_redo_cells(t):
    """the special-value runs of test_gpu_tiles.test_list_with_special_values reach every redo block
    of run_tile: per shaped launch of the type, over the lists that declare it and both modes, each
    of {whole, guarded} x {copy op, transposing op} x {ALPHA, AXPBY} holds at least one recovered
    element (flagged by the naive product, not NaN in both parts in the oracle's result: the redo
    must produce it) and one strip the main loop stores itself.  c64 (two elements a strip): per
    launch a redone strip that also holds an unflagged finite element and, in a guarded cell, a
    redone strip cut by the sub-tile's edge.  Per type: recoveries without an infinite input (the
    overflow branch) on `large` and `large_tr` under the huge scalars; a recovered element of a
    conjugating op per launch.  Counted by specials_common.redo_cells from the executor's work
    items, the data and the oracle alone; at most 15 % NaN parts per list.  An empty cell names
    itself: it is closed by another list or seed, never by dropping the cell."""
    from specials_common import total
    cells = {m: {} for m in _MODES}
    for name, (code, _, declared) in tile_lists.LISTS.items():
        if tile_lists.NAMES[code] != t:
            continue
        for m in _MODES:
            got, share = tile_lists.special_cells(name, m)
            assert not set(k[0] for k in got) - declared
            for k, c in got.items():
                cells[m].setdefault(k, c.__class__()).update(c)
    both = {}
    for m in _MODES:
        for k, c in cells[m].items():
            both.setdefault(k, c.__class__()).update(c)
    for k in sorted(both):
        print(t, *k, dict(both[k]))
    launches = sorted(REACHABLE[t] & set(tile_lists.SHAPED))
    assert {k[0] for k in both} == set(launches)
    empty = []
    for v in launches:
        fills = ("whole",) if (t, v) in _REDO_WHOLE_ONLY else ("whole", "guarded")
        for fill in fills:
            for mode in _OP_MODES.get(v, ("copy", "tr")):
                for kind in ("ALPHA", "AXPBY"):
                    c = total(both, launch=v, fill=fill, mode=mode, kind=kind)
                    for what in ("recovered", "not_redone"):
                        if c[what] == 0:
                            empty.append(f"{v} {fill} {mode} {kind}: no {what}")
        if (t, v) in _REDO_WHOLE_ONLY:
            assert total(both, launch=v, fill="guarded")["redone"] == 0, f"{t} {v} runs guarded sub-tiles"
        if v not in _NO_CONJ and total(both, launch=v, conj="conj")["recovered"] == 0:
            empty.append(f"{v}: no recovered element of a CONJ op")
        if t == "c64":
            if total(both, launch=v)["mixed"] == 0:
                empty.append(f"{v}: no redone strip with an unflagged finite element")
            if total(both, launch=v, fill="guarded")["partial"] == 0:
                empty.append(f"{v} guarded: no redone partial strip")
    for v in ("large", "large_tr"):
        # (the drawn data's 3e38 / 1e308 overflow some products already; the huge scalars add to them)
        if total(cells["huge"], launch=v)["overflow"] <= total(cells["drawn"], launch=v)["overflow"]:
            empty.append(f"{v} (huge): no recovery through the overflow branch")
    assert not empty, f"{t}: empty cells of the special-value runs:\n  " + "\n  ".join(empty)


def test_golden_case_routes():
    """a record, not an assertion (-s): the launches the golden cases' local, pack and unpack lists take"""
    import costa_amd
    from cases import all_cases
    seen = {}
    for case in all_cases():
        eff = [case.effective(k) for k in range(len(case.pairs))]
        for r in range(case.P):
            As = [case.layout_A(k, r, (1 << 40) + (k << 34)) for k in range(len(case.pairs))]
            Cs = [case.layout_C(k, r, (1 << 41) + (k << 34)) for k in range(len(case.pairs))]
            p = costa_amd.plan_export(As, Cs, r, case.P, [e[0] for e in eff], [e[1] for e in eff],
                                      [e[2] for e in eff])
            t = tile_lists.NAMES.get(int(As[0].dtype))
            if t is None or any(int(x.dtype) != int(As[0].dtype) for x in As + Cs):
                continue
            for kind, ops in (("local", p.local_ops), ("pack", p.pack_ops), ("unpack", p.unpack_ops)):
                for v in tile_lists.variants(As[0].dtype, ops, kind) if ops.size else ():
                    seen.setdefault((v, t), set()).add(case.name)
    lists = _declared_by_type()
    print()
    print(f"{'variant':22s}" + "".join(f"{t:>10s}" for t in REACHABLE) + "   (g = a golden case's list, t = a tile list)")
    for v in sorted(set().union(*REACHABLE.values())):
        cells = []
        for t in REACHABLE:
            c = ",".join(x for x, on in (("g", (v, t) in seen), ("t", v in lists[t])) if on)
            cells.append(c if v in REACHABLE[t] else ".")
        print(f"{v:22s}" + "".join(f"{c or '-':>10s}" for c in cells))
