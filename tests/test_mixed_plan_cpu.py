"""Planner of mixed-precision transforms on the CPU (no GPU needed).

A mixed pair (A and C of different element types: FLOAT <-> DOUBLE, CFLOAT <-> CDOUBLE) plans
exactly like the same-type transform of the same geometry: the same ops in the same order with
the same shapes, leading dimensions, scale / transpose / conj / slot bits and locality hints, the
same element offsets on every side, the same counts and displacements.  Only the byte offsets
differ: each side counts in its own element size, the package in the narrower of the two, and
each side's VEC flag follows its own byte alignment.
"""
import os
import subprocess

import numpy as np
import pytest

from casegen import BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, D, CF, Z = 0, 1, 2, 3
ESIZE = {S: 4, D: 8, CF: 8, Z: 16}
PAIRS = [(D, S), (S, D), (Z, CF), (CF, Z)]
NAMES = {S: "FLOAT", D: "DOUBLE", CF: "CFLOAT", Z: "CDOUBLE", 4: "INT32"}
BASE_A, BASE_C = 1 << 40, 1 << 41
M, N = 203, 157
VEC_SRC, VEC_DST = 0x4, 0x8
VEC = VEC_SRC | VEC_DST


def _plan(costa, ta, tc, op, grid, rank, alpha, beta, lld_pad=0, m=M, n=N, ab=(32, 48), cb=(40, 24)):
    pm, pn = grid
    am, an = (n, m) if op != "N" else (m, n)
    a = BC(am, an, ab[0], ab[1], pm=pm, pn=pn, lld_pad=lld_pad)
    c = BC(m, n, cb[0], cb[1], pm=pm, pn=pn, lld_pad=lld_pad)
    P = pm * pn
    A = a.make_layout(rank, BASE_A, P, ta)
    C = c.make_layout(rank, BASE_C, P, tc)
    return costa.plan_export([A], [C], rank, P, [op], [alpha], [beta])


def _same_bits(mixed, same):
    for f in ("nf", "ns", "lds", "ldd", "order"):
        assert (mixed[f] == same[f]).all(), f
    assert ((mixed["flags"] & ~np.uint32(VEC)) == (same["flags"] & ~np.uint32(VEC))).all()


def _elems(v, base, E):
    off = v.astype(np.int64) - base
    assert (off % E == 0).all()
    return off // E


def _vec_ok(ops, e_src, e_dst):
    """each side's VEC flag is set exactly when that side is 16-byte aligned in its own type"""
    src_al = (ops["src"] % 16 == 0) & (ops["lds"].astype(np.int64) * e_src % 16 == 0)
    dst_al = (ops["dst"] % 16 == 0) & (ops["ldd"].astype(np.int64) * e_dst % 16 == 0)
    assert (((ops["flags"] & VEC_SRC) != 0) == src_al).all()
    assert (((ops["flags"] & VEC_DST) != 0) == dst_al).all()


@pytest.mark.parametrize("grid", [(1, 1), (2, 2)], ids=["1rank", "2x2"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("ta,tc", PAIRS, ids=[f"{NAMES[a]}-{NAMES[c]}" for a, c in PAIRS])
def test_mixed_plan_equals_same_type_plan(costa, ta, tc, op, grid):
    alpha, beta = (1, 0) if op == "N" else (-0.5, 2.0)
    ea, ec = ESIZE[ta], ESIZE[tc]
    ep = min(ea, ec)
    P = grid[0] * grid[1]
    for rank in range(P):
        mx = _plan(costa, ta, tc, op, grid, rank, alpha, beta)
        for ts in (ta, tc):  # the same-type plan of the same geometry, in either type
            es = ESIZE[ts]
            sm = _plan(costa, ts, ts, op, grid, rank, alpha, beta)
            assert (mx.local_ops.size, mx.pack_ops.size, mx.unpack_ops.size) == \
                   (sm.local_ops.size, sm.pack_ops.size, sm.unpack_ops.size)
            for lst in ("local_ops", "pack_ops", "unpack_ops"):
                _same_bits(getattr(mx, lst), getattr(sm, lst))
            # element offsets: A's side in E_A, C's side in E_C, the package in min(E_A, E_C)
            assert (_elems(mx.local_ops["src"], BASE_A, ea) == _elems(sm.local_ops["src"], BASE_A, es)).all()
            assert (_elems(mx.local_ops["dst"], BASE_C, ec) == _elems(sm.local_ops["dst"], BASE_C, es)).all()
            assert (_elems(mx.pack_ops["src"], BASE_A, ea) == _elems(sm.pack_ops["src"], BASE_A, es)).all()
            assert (_elems(mx.pack_ops["dst"], 0, ep) == _elems(sm.pack_ops["dst"], 0, es)).all()
            assert (_elems(mx.unpack_ops["src"], 0, ep) == _elems(sm.unpack_ops["src"], 0, es)).all()
            assert (_elems(mx.unpack_ops["dst"], BASE_C, ec) == _elems(sm.unpack_ops["dst"], BASE_C, es)).all()
            for f in ("send_counts", "send_displs", "recv_counts", "recv_displs"):
                assert (getattr(mx, f) == getattr(sm, f)).all(), f
            assert (mx.send_elems, mx.recv_elems, mx.local_elems) == \
                   (sm.send_elems, sm.recv_elems, sm.local_elems)
        if P > 1:
            assert mx.pack_ops.size and mx.unpack_ops.size and mx.local_ops.size
        # the scalars are of C's type
        assert mx.scalars.dtype == np.dtype(costa.np_dtype(tc))
        assert mx.scalars[0] == alpha and mx.scalars[1] == beta
        _vec_ok(mx.local_ops, ea, ec)
        _vec_ok(mx.pack_ops, ea, ep)
        _vec_ok(mx.unpack_ops, ep, ec)


@pytest.mark.parametrize("lld_pad", [1, 2])
def test_vec_flags_follow_each_sides_alignment(costa, lld_pad):
    """64 x 48 in 32 x 16 blocks with lld = 64 + pad.  pad = 2: columns of the fp64 side are
    16-byte aligned (66 * 8 = 528), those of the fp32 side are not (66 * 4 = 264), so the mixed
    plan's flags differ from both same-type plans'.  pad = 1: neither side."""
    kw = dict(lld_pad=lld_pad, m=64, n=48, ab=(32, 16), cb=(32, 16))
    mx = _plan(costa, D, S, "N", (1, 1), 0, 1, 0, **kw).local_ops
    dd = _plan(costa, D, D, "N", (1, 1), 0, 1, 0, **kw).local_ops
    ss = _plan(costa, S, S, "N", (1, 1), 0, 1, 0, **kw).local_ops
    assert mx.size == dd.size == ss.size == 6
    _vec_ok(mx, 8, 4)
    if lld_pad == 2:
        assert ((dd["flags"] & VEC) == VEC).all() and ((ss["flags"] & VEC) == 0).all()
        assert ((mx["flags"] & VEC) == VEC_SRC).all()
        xm = _plan(costa, S, D, "N", (1, 1), 0, 1, 0, **kw).local_ops
        assert ((xm["flags"] & VEC) == VEC_DST).all()
    else:
        assert ((mx["flags"] & VEC) == 0).all()


def test_unsupported_pairs_are_named(costa):
    def lay(t, base):
        return BC(M, N, 32, 48).make_layout(0, base, 1, t)
    with pytest.raises(costa.CostaError, match="INT32.*DOUBLE"):
        costa.plan_export([lay(4, BASE_A)], [lay(D, BASE_C)], 0, 1)
    with pytest.raises(costa.CostaError, match="FLOAT.*CDOUBLE"):
        costa.plan_export([lay(S, BASE_A)], [lay(Z, BASE_C)], 0, 1)
    # one batch, two different pairs
    with pytest.raises(costa.CostaError, match="DOUBLE -> FLOAT and FLOAT -> DOUBLE") as e:
        costa.plan_export([lay(D, BASE_A), lay(S, BASE_A + (1 << 30))],
                          [lay(S, BASE_C), lay(D, BASE_C + (1 << 30))], 0, 1)
    assert e.value.code == 1  # COSTA_ERR_ARG
    # the GPU planner declines mixed pairs before it touches a GPU
    with pytest.raises(costa.CostaError, match="device planner"):
        costa.plan_export([lay(D, BASE_A)], [lay(S, BASE_C)], 0, 1, device=0)


def test_cpp_mixed_overloads_compile_and_link(tmp_path, costa):
    """costa::transform<Ta, Tc> (both forms) and the same-type overloads in one translation unit:
    no ambiguity, and the library exports the mixed instantiations"""
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <costa/layout.hpp>
#include <costa/transform.hpp>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>
template <typename Ta, typename Tc>
int run(int base) {
    std::vector<Ta> a(16);
    std::vector<Tc> c(16);
    auto A = costa::block_cyclic_layout<Ta>(4, 4, 2, 2, 1, 1, 4, 4, 1, 1, 'R', 0, 0, a.data(), 4, 'C', 0);
    auto C = costa::block_cyclic_layout<Tc>(4, 4, 2, 2, 1, 1, 4, 4, 1, 1, 'R', 0, 0, c.data(), 4, 'C', 0);
    int n = 0;
    try { costa::transform(A, C, nullptr); } catch (const costa::hip_error& e) {
        n += std::strstr(e.what(), "null communicator") != nullptr;
    }
    try { costa::transform(A, C, 'T', Tc(2), Tc(1), nullptr); } catch (const costa::hip_error& e) {
        n += std::strstr(e.what(), "null communicator") != nullptr;
    }
    return n == 2 ? 0 : base;
}
int main() {
    if (int r = run<double, float>(10)) return r;
    if (int r = run<float, double>(20)) return r;
    if (int r = run<std::complex<double>, std::complex<float>>(30)) return r;
    if (int r = run<std::complex<float>, std::complex<double>>(40)) return r;
    if (int r = run<double, double>(50)) return r;  // today's same-type overloads
    if (int r = run<float, float>(60)) return r;
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-Wall", f"-I{ROOT}/include", str(src), "-o", str(exe),
                    f"-L{os.path.dirname(costa.LIB_PATH)}", "-lcosta_amd",
                    f"-Wl,-rpath,{os.path.dirname(costa.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
