"""The ABI of triangular transforms (no GPU): the headers compile as C and C++ with the new
descriptor's size, both ScaLAPACK shim libraries export p?trmr2d, the C++ entry point links, and
the (uplo, diag, m, n) -> mask mapping the shims apply is the one MKL's p?trmr2d_ has."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONDA = "/opt/conda"
LIB = os.path.join(ROOT, "costa_amd", "lib")
MKL = ["-lmkl_scalapack_lp64", "-lmkl_blacs_intelmpi_lp64", "-lmkl_intel_lp64",
       "-lmkl_sequential", "-lmkl_core"]  # the link line of test_scalapack_dropin.py

need_mpi = pytest.mark.skipif(
    not (os.path.exists(f"{CONDA}/include/mpi.h") and os.path.exists(f"{CONDA}/lib/libmpi.so")
         and os.path.exists(os.path.join(LIB, "libcosta_amd_prefixed_scalapack.so"))),
    reason="MPICH / MKL ScaLAPACK or the shim library not available")

PROG = r'''
#include "costa_hip.h"
#include "costa/scalapack.h"
int main(void) {
    costa_tri_op_t t;
    costa_tri_plan_info_t info;
    (void)info;
    t.op.flags = COSTA_TRI_LE;
    t.diag = -3;
    void (*f)(COSTA_TRMR2D_ARGS(double)) = costa_pdtrmr2d_;
    void (*g)(COSTA_TRMR2D_ARGS(float)) = PCTRMR2D;
    (void)f; (void)g;
    return sizeof(costa_tile_op_t) == 40 && sizeof(costa_tri_op_t) == 48 && t.diag == -3 ? 0 : 1;
}
'''


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_headers_compile_as_c_and_cpp(tmp_path, lang):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text(PROG)
    obj = tmp_path / "t.o"
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", "-c", str(src), "-o", str(obj)],
                   check=True)
    # the sizes, in a program of its own (no library needed)
    src2 = tmp_path / ("s.c" if lang == "c" else "s.cpp")
    src2.write_text('#include "costa_hip.h"\nint main(void){return sizeof(costa_tile_op_t) == 40 && '
                    'sizeof(costa_tri_op_t) == 48 && COSTA_TRI_LE == 0x40u ? 0 : 1;}\n')
    exe = tmp_path / "s"
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", str(src2), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_python_descriptor_matches_the_header(costa):
    import ctypes
    assert costa.TRI_OP_DTYPE.itemsize == 48 == ctypes.sizeof(costa.TriOp)
    assert costa.TILE_OP_DTYPE.itemsize == 40
    assert costa.TRI_OP_DTYPE.fields["diag"][1] == 40
    assert costa.tri_cut() == 256
    bf, bs = costa.tri_subtile(costa.DOUBLE)
    assert bf > 0 and bs > 0
    assert list(costa.get_stats())[-1] == "tri_items"


@need_mpi
def test_shim_libraries_export_trmr2d():
    def syms(name):
        return subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, name)],
                              capture_output=True, text=True, check=True).stdout
    plain, pre = syms("libcosta_amd_scalapack.so"), syms("libcosta_amd_prefixed_scalapack.so")
    for t in "sdcz":
        base = f"p{t}trmr2d"
        for name in (base, base + "_", base + "__", base.upper()):
            assert f" T {name}\n" in plain, name
    for t in "sdczi":
        base = f"costa_p{t}trmr2d"
        for name in (base, base + "_", base + "__"):
            assert f" T {name}\n" in pre, name


def test_cpp_transform_triangular_compiles_and_links(tmp_path, costa):
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <costa/layout.hpp>
#include <costa/transform.hpp>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>
template <typename T>
int run() {
    std::vector<T> a(16), c(16);
    auto A = costa::block_cyclic_layout<T>(4, 4, 2, 2, 1, 1, 4, 4, 1, 1, 'R', 0, 0, a.data(), 4, 'C', 0);
    auto C = costa::block_cyclic_layout<T>(4, 4, 2, 2, 1, 1, 4, 4, 1, 1, 'R', 0, 0, c.data(), 4, 'C', 0);
    try { costa::transform_triangular<T>(A, C, 'T', 'L', -1, T(1), T(0), nullptr); }
    catch (const costa::hip_error& e) { return std::strstr(e.what(), "null communicator") ? 0 : 1; }
    return 2;
}
int main() {
    if (run<float>() || run<double>() || run<std::complex<float>>() || run<std::complex<double>>() ||
        run<int>()) return 1;
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


def build_trmr2d_check(tmp_path, with_costa):
    exe = tmp_path / ("trmr2d_gpu" if with_costa else "trmr2d_map")
    cmd = ["gcc", "-std=c99", "-O1", f"-I{CONDA}/include",
           os.path.join(ROOT, "tests", "scalapack", "trmr2d_check.c"), "-o", str(exe)]
    if with_costa:
        cmd += ["-DWITH_COSTA", f"-L{LIB}", "-lcosta_amd_prefixed_scalapack", "-lcosta_amd",
                f"-Wl,-rpath,{LIB}"]
    cmd += [f"-L{CONDA}/lib", *MKL, "-lmpi", "-lm",
            f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{CONDA}/lib"]
    subprocess.run(cmd, check=True, timeout=300)
    return exe


def run_mpi1(exe, arg):
    env = dict(os.environ, PATH=f"{CONDA}/bin:" + os.environ["PATH"])
    return subprocess.run([shutil.which("mpiexec", path=env["PATH"]) or f"{CONDA}/bin/mpiexec", "-n", "1",
                           str(exe), arg], capture_output=True, text=True, env=env, timeout=300)


def shim_mask(uplo, diag, m, n):
    """the mapping of include/costa/scalapack.h"""
    d = np.arange(n)[None, :] - np.arange(m)[:, None]
    unit = diag == "U"
    if uplo == "U":
        return d >= -max(m - n, 0) + unit
    return d <= max(n - m, 0) - unit


@need_mpi
def test_trmr2d_mapping_is_mkls(tmp_path):
    """MKL's p{s,d,c,z}trmr2d_ on one process: the set of elements it writes, for 5x3, 3x5 and 4x4
    at (ic, jc) = (3, 2) and every (uplo, diag), is the mask the shims ask for"""
    r = run_mpi1(build_trmr2d_check(tmp_path, False), "map")
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln[:2] in ("s ", "d ", "c ", "z ")]
    assert len(lines) == 4 * 3 * 2 * 2
    for t, uplo, diag, m, n, bits in lines:
        m, n = int(m), int(n)
        got = np.array([c == "1" for c in bits]).reshape(m, n)
        assert (got == shim_mask(uplo, diag, m, n)).all(), (t, uplo, diag, m, n, bits)
