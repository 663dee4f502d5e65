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
