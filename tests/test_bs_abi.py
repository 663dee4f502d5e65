"""The ABI of the block-scaled FP8 transforms (no GPU): the header compiles as C and as C++ with the new
declarations, the descriptor's size, layout and the enum values are mirrored in Python, and the library
exports the entry points."""
import ctypes
import subprocess

import pytest

from test_mx_abi import ROOT

PROG = r'''
#include "costa_hip.h"
int main(void) {
    int (*f)(costa_layout_t, costa_layout_t, char, const void*, const void*, const costa_block_scales_t*,
             const costa_block_scales_t*, int, costa_comm_t) = costa_hip_transform_block_scaled;
    int (*g)(costa_layout_t, costa_layout_t, char, const void*, const void*, const costa_block_scales_t*,
             const costa_block_scales_t*, int, costa_comm_t, void*) = costa_hip_transform_block_scaled_async;
    int (*e)(costa_dtype_t, costa_dtype_t, const costa_scaled_op_t*, int64_t, const void*, void*, const void*,
             int, const costa_block_scales_t*, const costa_block_scales_t*, int, int64_t, int64_t, int, int) =
        costa_hip_execute_tiles_block_scaled;
    int (*n)(int64_t*, int) = costa_hip_block_items;
    int (*o)(const costa_scaled_op_t*, int64_t, int, int, int64_t, int64_t) = costa_hip_block_check_ops;
    int (*c)(const costa_block_scales_t*, int64_t, int64_t) = costa_hip_block_check_scales;
    costa_block_scales_t s;
    s.data = 0; s.block_rows = 1; s.block_cols = 128; s.row_stride = 3; s.col_stride = 1;
    (void)f; (void)g; (void)e; (void)n; (void)o; (void)c; (void)s;
    return 0;
}
'''

SIZES = r'''
#include <stddef.h>
#include <stdio.h>
#include "costa_hip.h"
int main(void) {
    printf("%d %d %d %d %d %d %d %d\n", (int)sizeof(costa_block_scales_t), (int)offsetof(costa_block_scales_t, data),
           (int)offsetof(costa_block_scales_t, block_rows), (int)offsetof(costa_block_scales_t, block_cols),
           (int)offsetof(costa_block_scales_t, row_stride), (int)offsetof(costa_block_scales_t, col_stride),
           COSTA_BLOCK_EXACT, COSTA_BLOCK_POW2);
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
    size, o_data, o_br, o_bc, o_rs, o_cs, exact, pow2 = map(int, out)
    B = costa.BlockScales
    assert size == 32 == ctypes.sizeof(B)
    assert (o_data, o_br, o_bc, o_rs, o_cs) == (B.data.offset, B.block_rows.offset, B.block_cols.offset,
                                                B.row_stride.offset, B.col_stride.offset) == (0, 8, 12, 16, 24)
    assert (exact, pow2) == (costa.BLOCK_EXACT, costa.BLOCK_POW2) == (0, 1)


def test_library_exports_the_entry_points(costa):
    syms = subprocess.run(["nm", "-D", "--defined-only", costa.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for name in ("costa_hip_transform_block_scaled", "costa_hip_transform_block_scaled_async",
                 "costa_hip_execute_tiles_block_scaled", "costa_hip_block_items", "costa_hip_block_check_ops",
                 "costa_hip_block_check_scales"):
        assert f" T {name}\n" in syms, name


def test_python_names(costa):
    for name in ("BlockScales", "block_scales", "transform_block_scaled", "execute_tiles_block_scaled",
                 "block_items", "block_check_ops", "block_check_scales"):
        assert name in costa.__all__ and callable(getattr(costa, name)), name
    d = costa.BlockScales(0x1000, 1, 128, 3, 5)
    assert (d.data, d.block_rows, d.block_cols, d.row_stride, d.col_stride) == (0x1000, 1, 128, 3, 5)
    with pytest.raises(ValueError):
        costa.block_scales(object(), (128, 128))
    with pytest.raises(ValueError):
        costa.block_scales(None, (64, 64))
