"""The ABI of the amax outputs (no GPU): the header compiles as C and as C++ with the new entry
points' signatures, the scaled descriptor keeps its size, and the library exports the entry points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r'''
#include "costa_hip.h"
int main(void) {
    int (*f)(costa_layout_t, costa_layout_t, char, const void*, const void*, const void*, const void*,
             void*, void*, costa_comm_t) = costa_hip_transform_amax;
    int (*g)(costa_layout_t, costa_layout_t, char, const void*, const void*, const void*, const void*,
             void*, void*, costa_comm_t, void*) = costa_hip_transform_amax_async;
    int (*h)(costa_layout_t, void*, void*, costa_comm_t) = costa_hip_layout_amax;
    int (*k)(costa_layout_t, void*, void*, costa_comm_t, void*) = costa_hip_layout_amax_async;
    int (*e)(costa_dtype_t, costa_dtype_t, const costa_scaled_op_t*, int64_t, const void*, void*,
             const void*, int, const void*, const void*, void*, void*, int) = costa_hip_execute_tiles_amax;
    int (*n)(int64_t*, int) = costa_hip_amax_items;
    (void)f; (void)g; (void)h; (void)k; (void)e; (void)n;
    return sizeof(costa_scaled_op_t) == 48 ? 0 : 1;
}
'''


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_as_c_and_cpp(tmp_path, lang):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text(PROG)
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)
    # the descriptor's size, in a program of its own (no library needed)
    src2 = tmp_path / ("s.c" if lang == "c" else "s.cpp")
    src2.write_text('#include "costa_hip.h"\nint main(void){return sizeof(costa_scaled_op_t) == 48 && '
                    'sizeof(costa_tile_op_t) == 40 ? 0 : 1;}\n')
    exe = tmp_path / "s"
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", str(src2), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_library_exports_the_amax_entry_points(costa):
    syms = subprocess.run(["nm", "-D", "--defined-only", costa.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for name in ("costa_hip_transform_amax", "costa_hip_transform_amax_async", "costa_hip_layout_amax",
                 "costa_hip_layout_amax_async", "costa_hip_execute_tiles_amax", "costa_hip_amax_items"):
        assert f" T {name}\n" in syms, name


def test_python_names(costa):
    for name in ("transform_amax", "layout_amax", "execute_tiles_amax", "amax_items"):
        assert name in costa.__all__ and callable(getattr(costa, name)), name
