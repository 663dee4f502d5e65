"""The ABI of scaled transforms (no GPU): the header compiles as C and as C++ with the new
descriptor's size and flag, and the library exports the new entry points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r'''
#include "costa_hip.h"
int main(void) {
    costa_scaled_op_t t;
    costa_scaled_plan_info_t info;
    int (*f)(costa_layout_t, costa_layout_t, char, const void*, const void*, const void*, const void*,
             costa_comm_t) = costa_hip_transform_scaled;
    int (*g)(costa_dtype_t, costa_dtype_t, int*, int*) = costa_hip_scaled_subtile;
    (void)info; (void)f; (void)g;
    t.op.flags = COSTA_SCALED_F_ROWS;
    t.row0 = 3;
    t.col0 = 5;
    return sizeof(costa_tile_op_t) == 40 && sizeof(costa_scaled_op_t) == 48 && t.row0 + t.col0 == 8 ? 0 : 1;
}
'''


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_as_c_and_cpp(tmp_path, lang):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text(PROG)
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)
    # the sizes, in a program of its own (no library needed)
    src2 = tmp_path / ("s.c" if lang == "c" else "s.cpp")
    src2.write_text('#include <stddef.h>\n#include "costa_hip.h"\nint main(void){return '
                    'sizeof(costa_scaled_op_t) == 48 && offsetof(costa_scaled_op_t, row0) == 40 && '
                    'offsetof(costa_scaled_op_t, col0) == 44 && COSTA_SCALED_F_ROWS == 0x80u && '
                    'sizeof(costa_scaled_plan_info_t) == sizeof(costa_plan_info_t) + 16 ? 0 : 1;}\n')
    exe = tmp_path / "s"
    subprocess.run([*cc, "-Wall", "-Werror", f"-I{ROOT}/include", str(src2), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_library_exports_the_scaled_entry_points(costa):
    syms = subprocess.run(["nm", "-D", "--defined-only", costa.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    for name in ("costa_hip_transform_scaled", "costa_hip_transform_scaled_async",
                 "costa_hip_plan_export_scaled", "costa_hip_execute_tiles_scaled",
                 "costa_hip_scaled_subtile", "costa_hip_scaled_items"):
        assert f" T {name}\n" in syms, name
