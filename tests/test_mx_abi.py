"""The ABI of the MX block-scaled transforms (no GPU): the header compiles as C and as C++ with the new
declarations, the descriptor's size and the enum values are mirrored in Python, and the library exports
the entry points."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r'''
#include "costa_hip.h"
int main(void) {
    int (*f)(costa_layout_t, costa_layout_t, char, const void*, const void*, const costa_mx_scales_t*,
             const costa_mx_scales_t*, int, costa_comm_t) = costa_hip_transform_mx;
    int (*g)(costa_layout_t, costa_layout_t, char, const void*, const void*, const costa_mx_scales_t*,
             const costa_mx_scales_t*, int, costa_comm_t, void*) = costa_hip_transform_mx_async;
    int (*e)(costa_dtype_t, costa_dtype_t, const costa_scaled_op_t*, int64_t, const void*, void*, const void*,
             int, const costa_mx_scales_t*, const costa_mx_scales_t*, int, int64_t, int64_t, int, int) =
        costa_hip_execute_tiles_mx;
    int (*n)(int64_t*, int) = costa_hip_mx_items;
    costa_mx_scales_t s;
    s.data = 0; s.axis = COSTA_MX_COLS; s.block_stride = 1; s.line_stride = 7;
    (void)f; (void)g; (void)e; (void)n; (void)s;
    return 0;
}
'''

SIZES = r'''
#include <stddef.h>
#include <stdio.h>
#include "costa_hip.h"
int main(void) {
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof(costa_mx_scales_t), (int)offsetof(costa_mx_scales_t, data),
           (int)offsetof(costa_mx_scales_t, axis), (int)offsetof(costa_mx_scales_t, block_stride),
           (int)offsetof(costa_mx_scales_t, line_stride), COSTA_MX_ROWS, COSTA_MX_COLS, COSTA_MX_FLOOR,
           COSTA_MX_CEIL);
    return 0;
}
'''


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_and_python_mirrors_it(costa, tmp_path, lang):
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
    ext = "c" if lang == "c" else "cpp"
    src = tmp_path / f"t.{ext}"
    src.write_text(PROG)
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)
    src2 = tmp_path / f"s.{ext}"
    src2.write_text(SIZES)
    exe = tmp_path / "s"
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", str(src2), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    size, o_data, o_axis, o_bs, o_ls, rows, cols, floor, ceil = map(int, out)
    M = costa.MxScales
    assert size == 32 == ctypes.sizeof(M)
    assert (o_data, o_axis, o_bs, o_ls) == (M.data.offset, M.axis.offset, M.block_stride.offset,
                                            M.line_stride.offset)
    assert (rows, cols, floor, ceil) == (costa.MX_ROWS, costa.MX_COLS, costa.MX_FLOOR, costa.MX_CEIL) == (0, 1, 0, 1)


def test_library_exports_the_mx_entry_points(costa):
    syms = subprocess.run(["nm", "-D", "--defined-only", costa.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for name in ("costa_hip_transform_mx", "costa_hip_transform_mx_async", "costa_hip_execute_tiles_mx",
                 "costa_hip_mx_items", "costa_hip_mx_check_ops", "costa_hip_mx_check_scales"):
        assert f" T {name}\n" in syms, name


def test_python_names(costa):
    for name in ("MxScales", "mx_scales", "transform_mx", "execute_tiles_mx", "mx_items"):
        assert name in costa.__all__ and callable(getattr(costa, name)), name
    d = costa.MxScales(0x1000, costa.MX_COLS, 3, 5)
    assert (d.data, d.axis, d.block_stride, d.line_stride) == (0x1000, 1, 3, 5)
