"""GPU parity of one batched tile launch against the oracle, on the op lists of tests/tile_lists.py:
random lists that mix every work class of the executor -- tiny ops (one wavefront each, copy and LDS
transpose), the medium and large sub-tile shapes (copy and transposing lists), the class boundaries
(engine.cpp tiny_copy_budget / kTinyLdsBytes), thin ops (nf = 1, ns = 1), padded strides, unaligned
offsets, every scale kind -- and lists made for one launch variant of tile_kernels.hip each (the
square, 32 x 32, all-whole, skew and destination-block-group routes, with and without a beta*C op).

Every list is in the registry tile_lists.LISTS with the launches it exists to exercise.  Before the
launch each test asserts, on the host, that tile_kernels.hip launch_t would issue those launches for
the list (tile_lists.check_route: engine.cpp build_work's split through costa_hip_work_export): a
dispatch rule that moves fails the test instead of retargeting it.

Each op is the reference's copy_and_transform (memory_utils.hpp:339-412); the oracle executes
the same list op by op (oracle.exec_tile_ops).  Bit-exact: integers and finite floats with
contraction off on both sides, compared over the whole destination buffer, the elements
between and after the ops included.
"""
import numpy as np
import pytest

import oracle
import specials_common
import tile_lists

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# registry prefix -> the test that runs its lists (tests/test_tile_variants_cpu.py: every list has one)
TESTS = {"mixed": "test_mixed_tile_list", "medium": "test_medium_shape_list",
         "unaligned": "test_unaligned_large_list", "square": "test_square_shape_list",
         "full": "test_full_tile_list", "phase": "test_wavefront_transposes_every_phase",
         "noax": "test_no_axpby_list", "wave": "test_wavefront_only_list", "group": "test_group_list",
         "skew": "test_skew_list"}


def registry(prefix):
    """parametrisation over the registry lists `prefix[...]`: one case per list, the id its key"""
    keys = [n[len(prefix) + 1:-1] for n in tile_lists.LISTS if n.startswith(prefix + "[")]
    return pytest.mark.parametrize("name", [f"{prefix}[{k}]" for k in keys], ids=keys)


@pytest.fixture(scope="module")
def gpu(costa):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return costa


def run_list(gpu, name):
    """the route first (host), then one execute_tiles launch against the oracle, byte for byte over
    the whole destination buffer"""
    code, ops, src, dst0, scal, _ = tile_lists.build(name)
    tile_lists.check_route(name, ops)
    dt = oracle.NP[code]
    E = np.dtype(dt).itemsize
    exp = dst0.copy()
    oracle.exec_tile_ops(code, ops, scal, src.ctypes.data, exp.ctypes.data)

    d_src = torch.from_numpy(src.view(np.uint8).copy()).cuda()
    d_dst = torch.from_numpy(dst0.view(np.uint8).copy()).cuda()
    gpu.execute_tiles(code, ops, scal, d_src.data_ptr(), d_dst.data_ptr())
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy().view(dt)
    n = dst0.size
    bad = np.flatnonzero((got.view(np.uint8).reshape(n, E) != exp.view(np.uint8).reshape(n, E)).any(1))
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[0]}: {got[bad[0]]} vs {exp[bad[0]]}"


# ---------------------------------------------------------------------------- special values
# The real types' lists of test_list_with_special_values: one per shaped launch and per wavefront /
# group launch of DESIGN §4a's table (no redo path there: inf / NaN through the arithmetic, and with
# them in C, "ALPHA / ZERO ops do not read C" on every launch).  test_tile_variants_cpu.py asserts
# that each list declares its launch and that no launch of the type is left out.
REAL_SPECIALS = {
    "f32": {"large": "mixed[copy-f32]", "large_tr": "mixed[1-f32]", "medium_tr": "medium[f32-64]",
            "medium_tr_full": "medium[f32-64-full]", "small32_tr": "medium[f32-32]",
            "skew": "skew[off16-f32]", "skew_wide": "skew[wide-off16-f32]",
            "cblock_N": "group[N-f32]", "cblock_N+pieces": "group[N+p-f32]",
            "cblock_T": "group[T-f32]", "cblock_T+pieces": "group[T+p-f32]",
            "cblock_Nax": "group[Nax-f32]", "cblock_Nax+pieces": "group[Nax+p-f32]",
            "cblock_Tax": "group[Tax-f32]", "cblock_Tax+pieces": "group[Tax+p-f32]",
            "tiny_N": "wave[N-f32]", "tiny_T": "wave[T-f32]", "tiny_Nax": "unaligned[copy-f32]",
            "tiny_Tax": "phase[1-f32]"},
    "f64": {"large": "mixed[copy-f64]", "large_tr": "mixed[1-f64]", "small_tr": "square[1-f64]",
            "medium_tr": "medium[f64-mix]", "small32_tr": "medium[f64-32]", "skew": "skew[off64-f64]",
            "cblock_N": "group[N-f64]", "cblock_N+pieces": "group[N+p-f64]",
            "cblock_T": "group[T-f64]", "cblock_T+pieces": "group[T+p-f64]",
            "cblock_Nax": "group[Nax-f64]", "cblock_Nax+pieces": "group[Nax+p-f64]",
            "cblock_Tax": "group[Tax-f64]", "cblock_Tax+pieces": "group[Tax+p-f64]",
            "tiny_N": "wave[N-f64]", "tiny_T": "wave[T-f64]", "tiny_Nax": "unaligned[copy-f64]",
            "tiny_Tax": "unaligned[mixed-f64]"},
}
# every c64 / c128 list in both modes ("huge": alpha * x overflows, the recovery's branch without an
# infinite input); the real types' table in "drawn" mode
SPECIAL_CASES = [(n, m) for n, (c, _, _) in tile_lists.LISTS.items() if tile_lists.NAMES[c] in ("c64", "c128")
                 for m in ("drawn", "huge")]
SPECIAL_CASES += [(n, "drawn") for t in REAL_SPECIALS for n in dict.fromkeys(REAL_SPECIALS[t].values())]


@pytest.mark.parametrize("name,mode", SPECIAL_CASES, ids=[f"{n}-{m}" for n, m in SPECIAL_CASES])
def test_list_with_special_values(gpu, name, mode):
    """the registry list with oracle.add_specials over its source and initial destination (about one
    element in 8 with parts from {+-inf, NaN, +-0, huge, -3, 0.5}): the complex shaped launches then
    skip the stores of the strips whose naive products come out NaN in both parts and recompute them
    after the main loop (the `redo` blocks of run_tile), next to strips they store as usual.  The
    route first, one launch, then every real part of the whole destination bit-equal to the oracle's
    or NaN on both sides (specials_common.assert_parts; at most 15 % of the written parts may be
    NaN, asserted on the expected buffer).  test_tile_variants_cpu.py counts, from the data and the
    oracle, that per launch x whole / guarded x copy / transpose x ALPHA / AXPBY these runs hold
    recovered elements and strips left alone."""
    code, ops, src, dst0, scal, _ = tile_lists.build(name, mode)
    tile_lists.check_route(name, ops)
    exp, mask = tile_lists.expected(code, ops, scal, src, dst0)
    share = specials_common.assert_nan_share(exp, mask, f"{name} {mode}")
    d_src = torch.from_numpy(src.view(np.uint8).copy()).cuda()
    d_dst = torch.from_numpy(dst0.view(np.uint8).copy()).cuda()
    gpu.execute_tiles(code, ops, scal, d_src.data_ptr(), d_dst.data_ptr())
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy().view(dst0.dtype)
    print(f"{name} {mode}: {share:.1%} of the written real parts are NaN")
    specials_common.assert_parts(got, exp, f"{name} {mode}")


@registry("mixed")
def test_mixed_tile_list(gpu, name):
    """240 random ops over every class; seeds 1-3 transposing lists (`large_tr`), "copy" copy-only
    (`large`); complex types' small ops on the wavefront launch that reads C (`tiny_Tax` / `tiny_Nax`)"""
    run_list(gpu, name)


@registry("medium")
def test_medium_shape_list(gpu, name):
    """a transposing list of >= 4096 aligned ops between half a medium and half a large
    sub-tile (engine.cpp kMinMediumOps: the medium shape only runs for lists this long), with
    every scale kind and padded strides (`medium_tr`); full: every op a whole medium sub-tile and no
    beta*C op (the `medium_tr_full` launch); nb = 32: the medium class on 32 x 32 sub-tiles
    (`small32_tr`, every type); f64-mix: fp64 ops of exactly 32 x 64 mixed with ragged ones (whole and
    guarded `medium_tr` sub-tiles; f64-48 has ragged ones only), -noax without a beta*C op; i32-24 is the negative case: 24 x 24 ops would part-fill every 32 x 32
    sub-tile, so build_work gives no medium launch (n_medium = 0) and the ops run as
    destination-block groups with wavefront pieces (`cblock_Tax+pieces`); bit-exact against the oracle"""
    run_list(gpu, name)


@registry("unaligned")
def test_unaligned_large_list(gpu, name):
    """large ops whose columns are not 16-byte aligned on one side or both (odd lld for 8-byte
    types, lld % 4 != 0 for 4-byte ones): the large shape's element-wise path
    (tile_kernels.hip run_tile_elem) of `large_tr` (mixed) and `large` (copy), full and ragged
    sub-tiles, every scale kind; their edges on `tiny_Tax` / `tiny_Nax`; bit-exact against the oracle"""
    run_list(gpu, name)


@registry("square")
def test_square_shape_list(gpu, name):
    """a transposing list whose large ops all fit 64 x 64 (nb = 64 blocks): the large ops run on
    the square variant of the transposing shape (engine.cpp build_work, tile_kernels.hip
    `small_tr`); copy-mode ops, padded and unaligned strides, every scale kind (conjugation for
    complex types), plus small ops on the wavefront path; bit-exact against the oracle"""
    run_list(gpu, name)


@registry("full")
def test_full_tile_list(gpu, name):
    """a transposing list whose large ops are all aligned whole multiples of the large sub-tile (c128
    64 x 128, fp64 64 x 128) with leading dimensions on the 64-byte grid: engine.cpp
    work_split::full.  c128: the `large_tr_full` launch, a 256-thread kernel of its own; one ragged
    128 x 20 op keeps the list off the square shape, and small ops run the wavefront launch in the
    same call; c128-noax: the same without a beta*C op.  fp64: `large_tr_full` is `large_tr` itself,
    here with every sub-tile whole.  f32-mix / i32-mix: aligned transposing ops, whole multiples of 128 x 128
    and ragged ones (`large_tr`: whole sub-tiles of transposing ops, full = 0).  Copy and transpose ops, every scale kind (conjugation for c128);
    bit-exact against the oracle"""
    run_list(gpu, name)


@registry("phase")
def test_wavefront_transposes_every_phase(gpu, name):
    """wavefront transposes (`tiny_Tax`) of 4-byte elements into destination columns at every 16-byte
    phase (r4 measured a variant that writes aligned 16-byte chunks with element-wise heads and tails;
    this pins the edges any such variant must get right): every destination offset mod 4, leading
    dimensions ns .. ns + 3 (each column starting at another phase), heights 1 .. 160 (all edges, no
    full chunk, a single chunk), widths 1 .. 64, ops the host cuts into pieces, every scale kind;
    neighbouring ops' destination columns share 16-byte chunks (no op may write outside its own
    elements).  Bit-exact against the oracle."""
    run_list(gpu, name)


@registry("noax")
def test_no_axpby_list(gpu, name):
    """the mixed recipe without a beta*C op (scale kinds 0-2): `large` and `large_tr` never load C;
    complex types' small ops run tiny_kernel's AX = false instantiations (`tiny_N`, `tiny_T`)"""
    run_list(gpu, name)


@registry("wave")
def test_wavefront_only_list(gpu, name):
    """small ops for the wavefront launch alone, no beta*C op: `tiny_N` and `tiny_T` of every type
    (the real types' too, whose small ops the other lists fuse into group launches)"""
    run_list(gpu, name)


@registry("group")
def test_group_list(gpu, name):
    """ragged destination blocks tiled exactly by their ops: every instantiation of cblock_kernel
    (`cblock_{N,T}[ax]`), alone and with wavefront pieces in the launch's tail (`+pieces`), the
    elements between the blocks untouched"""
    run_list(gpu, name)


@registry("skew")
def test_skew_list(gpu, name):
    """transposes into destination columns off the 16-byte grid, or on it and off the 64-byte one,
    with a leading dimension above the group budget: `skew`, and `skew_wide` when 4-byte sources are
    off the 16-byte grid too; ragged heights, merged ops, beta*C ops, shared granules, guard after"""
    run_list(gpu, name)
