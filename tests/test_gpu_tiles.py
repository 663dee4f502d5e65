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
