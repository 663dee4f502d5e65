// Internal engine interface: type-erased layouts, the tile planner and the executor.
#pragma once

#include <costa/layout.hpp>
#include <costa_hip.h>

#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "tile_op.hpp"

namespace costa {
namespace engine {

// bytes of one element; COSTA_FP4_E2M1 (half a byte) and the FP6 types (three quarters) throw
// COSTA_ERR_ARG naming the type
size_t dtype_size(costa_dtype_t t);
// ... of any type, in quarter-bytes (tile_op.hpp esize): wherever an address or a byte count of a
// layout side is formed
esize elem_size(costa_dtype_t t);
bool dtype_is_complex(costa_dtype_t t);
bool dtype_is_half(costa_dtype_t t);  // the 2-byte types: COSTA_HALF, COSTA_BFLOAT16
// the type of alpha / beta and of the arithmetic of an (A, C) pair: C's type, FLOAT when A or C is
// a 2-byte type
costa_dtype_t compute_dtype(costa_dtype_t src, costa_dtype_t dst);
// H -> H of one H, FLOAT -> H, H -> FLOAT (H a 2-byte type): the pairs of half_kernels.hip
bool half_pair(costa_dtype_t src, costa_dtype_t dst);
// the 1-byte types (COSTA_FP8_E4M3, COSTA_FP8_E5M2; compute_dtype is FLOAT for them too) and their
// pairs Q -> Q of one Q, FLOAT -> Q, Q -> FLOAT: the pairs of fp8_kernels.hip
bool dtype_is_fp8(costa_dtype_t t);
bool fp8_pair(costa_dtype_t src, costa_dtype_t dst);
// the packed sub-byte types (compute_dtype is FLOAT): COSTA_FP4_E2M1, two elements per byte, and
// COSTA_FP6_E2M3 / COSTA_FP6_E3M2, four elements per three bytes; packed_group() is the elements of
// one packing group (2, 4; 0 for every other type) and packed_rule() the name of the rule that keeps
// a tile from splitting one ("FP4 pair", "FP6 quad").  Their pairs P -> P, FLOAT -> P, P -> FLOAT:
// MX transforms only (costa_hip.h, "MXFP4", "MXFP6"), planned on the host
bool dtype_is_fp4(costa_dtype_t t);
bool dtype_is_fp6(costa_dtype_t t);
bool dtype_is_packed(costa_dtype_t t);
int packed_group(costa_dtype_t t);
const char* packed_rule(costa_dtype_t t);
bool packed_pair(costa_dtype_t src, costa_dtype_t dst);
// a package is counted in units of this many bytes: its elements, or single bytes when it holds a
// packed type (A holds FP4 or FP6), so that no count, displacement or round boundary falls inside a
// byte
size_t pkg_unit_size(costa_dtype_t pkg);
int64_t pkg_units(costa_dtype_t pkg, int64_t elems);
// element type of the packages of an (A, C) plan: the narrower of the two; A's for FP8 pairs
// (FLOAT -> Q carries FLOAT: its source is not rounded before the arithmetic)
costa_dtype_t plan_pkg_dtype(costa_dtype_t src, costa_dtype_t dst);

// One local block, element-type erased.  Intervals are in the layout's own (untransposed)
// global coordinates; `data` points at its first element.
struct eblock {
    interval rows, cols;
    char* data = nullptr;
    int ld = 0;
};

// A grid_layout<T> with the element type erased (owners row-major, like the reference's
// ranks[i][j]).  Plans are built from these.
struct elayout {
    costa_dtype_t dtype = COSTA_DOUBLE;
    std::vector<int> rows_split, cols_split;
    std::vector<int> owners;
    int n_ranks = 1;
    char ordering = 'C';
    std::vector<eblock> blocks;
    uint64_t hash = 0;   // content hash (plan-cache key); 0 = not computed yet
    uint64_t hash2 = 0;  // a second, independently seeded content hash (verified on a cache hit)

    int nbr() const { return int(rows_split.size()) - 1; }
    int nbc() const { return int(cols_split.size()) - 1; }
};

template <typename T>
costa_dtype_t dtype_of();

template <typename T>
elayout erase(const grid_layout<T>& L);

// content hash of a layout (splits, owners, ordering, every block's intervals/pointer/ld)
uint64_t layout_hash(const elayout& L);
// both content hashes (h1 == layout_hash(L)), stored in L.hash / L.hash2 by set_layout_hash
void layout_hashes(const elayout& L, uint64_t& h1, uint64_t& h2);
void set_layout_hash(elayout& L);

// scalars (alpha, beta) of one layout pair, stored as raw bytes of the dtype
struct scal {
    std::array<unsigned char, 16> alpha{};
    std::array<unsigned char, 16> beta{};
};

// one (A -> C) pair of a transform
struct job {
    const elayout* A = nullptr;
    const elayout* C = nullptr;
    char trans = 'N';
    scal s;
    // triangular transforms: 'U' keeps target elements with j - i >= k, 'L' those with j - i <= k
    // (i, j from the first row / column of C's layout), 'A' (the default) all of them
    char uplo = 'A';
    int k = 0;
    // scaled transforms (costa_hip_transform_scaled): every LOCAL and UNPACK op carries its target
    // coordinates; the vectors (device arrays of the compute type, either may be null) are arguments
    // of the call, not part of the plan or of its cache key
    bool scaled = false;
    const void* row_scale = nullptr;
    const void* col_scale = nullptr;
    // amax outputs (costa_hip_transform_amax): device arrays updated by the LOCAL / UNPACK kernels of
    // a scaled job; arguments of the call like the scales (with one of them both scales may be null)
    void* row_amax = nullptr;
    void* col_amax = nullptr;
    // MX block-scaled transforms (costa_hip_transform_mx): a scaled job whose LOCAL / UNPACK lists run
    // on mx_kernel; the descriptors (data == NULL: none) and the rounding mode are arguments of the
    // call like the vectors above
    bool mx = false;
    costa_mx_scales_t a_scales{};
    costa_mx_scales_t c_scales{};
    int mx_rounding = 0;
    // ... and, for costa_hip_transform_mx_sr, the seed of the call's stochastic rounding (of the call,
    // not of the plan: the cache key does not see it)
    bool mx_sr = false;
    uint64_t mx_seed = 0;
    // ... and, for costa_hip_transform_mx_dual, the second target and its descriptor: the plan is that of
    // (A, C, trans), every LOCAL / UNPACK op gets a twin in Ct and the lists run on mx_dual_kernel.  Ct is
    // part of the plan's cache key (the twins hold its addresses)
    const elayout* Ct = nullptr;
    costa_mx_scales_t ct_scales{};
    // block-scaled FP8 transforms (costa_hip_transform_block_scaled): likewise a scaled job, its lists
    // on block_kernel
    bool blk = false;
    costa_block_scales_t a_blocks{};
    costa_block_scales_t c_blocks{};
    int blk_rounding = 0;
};

// The three tile-op lists of one rank plus the exchange geometry.  Addresses of pack
// destinations and unpack sources are byte offsets into the send / receive buffers.
struct plan {
    costa_dtype_t dtype = COSTA_DOUBLE;      // C's element type: the scalars and all arithmetic
    // Mixed-precision plans (A's type differs from C's): local ops read src_dtype and write dtype;
    // the package holds pkg_dtype, the narrower of the two, so the converting list is PACK
    // (src_dtype -> pkg_dtype) for narrowing pairs and UNPACK (pkg_dtype -> dtype) for widening
    // ones, and the other list is a same-type list.  Same-type plans: all three equal.
    costa_dtype_t src_dtype = COSTA_DOUBLE;  // A's element type
    costa_dtype_t pkg_dtype = COSTA_DOUBLE;  // element type of the send / receive packages
    bool mixed() const { return src_dtype != dtype; }
    // Half-precision plans (A or C of a 2-byte type H; H -> H, FLOAT -> H, H -> FLOAT): pkg_dtype is
    // H and all three lists run on the converting family of half_kernels.hip, the same-type H -> H
    // lists included (tile_kernels.hip has no 2-byte shape); the scalars are fp32.
    bool half() const { return dtype_is_half(src_dtype) || dtype_is_half(dtype); }
    // every list of the plan runs on a converting family, or (mixed, not half) LOCAL and one of
    // PACK / UNPACK
    // FP8 plans (A or C of a 1-byte type Q; Q -> Q, FLOAT -> Q, Q -> FLOAT): pkg_dtype is A's type.
    // LOCAL and UNPACK run on the converting family of fp8_kernels.hip; PACK is a byte copy of
    // 1-byte tiles on it when A holds Q, and a same-type FLOAT list on tile_kernel when A is FLOAT.
    bool fp8() const { return dtype_is_fp8(src_dtype) || dtype_is_fp8(dtype); }
    // packed plans (A or C of COSTA_FP4_E2M1 or an FP6 type, scaled plans of MX calls only): the package
    // holds A's type; a packed package's PACK list is a byte copy on the FP8 family's Q -> Q kernel
    bool packed() const { return dtype_is_packed(src_dtype) || dtype_is_packed(dtype); }
    bool converting() const { return mixed() || half() || fp8() || packed(); }
    costa_dtype_t scalar_dtype() const { return compute_dtype(src_dtype, dtype); }
    int rank = 0, n_ranks = 1;
    std::vector<costa_tile_op_t> local_ops, pack_ops, unpack_ops;
    // triangular transforms: the LOCAL and UNPACK ops of the tiles the mask's diagonal cuts (their
    // pack ops are ordinary dense copies in pack_ops); empty for every other plan
    std::vector<costa_tri_op_t> local_tri, unpack_tri;
    // scaled transforms: every LOCAL and UNPACK op, in the ordinary plan's order (local_ops and
    // unpack_ops are then empty; pack_ops and the exchange geometry are the ordinary plan's)
    bool scaled = false;
    std::vector<costa_scaled_op_t> local_scaled, unpack_scaled;
    std::vector<int64_t> send_counts, send_displs, recv_counts, recv_displs;  // elements (pkg_units)
    int64_t send_elems = 0, recv_elems = 0, local_elems = 0;
    std::vector<scal> slots;
    // algorithmic HBM bytes of each list (read + write (+ read of C when beta != 0))
    int64_t local_bytes = 0, pack_bytes = 0, unpack_bytes = 0;
};

// per-job transform parameters, validated as the reference's transform does (plan.cpp)
struct job_params {
    bool transpose, conj, a_cm, c_cm;
    uint32_t kind_copy, kind_tr;  // scale kind of ops that copy / transpose
};
std::vector<job_params> check_jobs(const std::vector<job>& jobs, int n_ranks, costa_dtype_t& dtype);
// the same for batches whose A and C may differ in element type: every job shares one
// (A dtype, C dtype) pair, equal or one of FLOAT <-> DOUBLE, CFLOAT <-> CDOUBLE; the scale kinds
// are evaluated in C's type
std::vector<job_params> check_jobs(const std::vector<job>& jobs, int n_ranks,
                                   costa_dtype_t& src_dtype, costa_dtype_t& dst_dtype);
const char* dtype_name(costa_dtype_t t);
// whether some job of the batch is masked (uplo 'U' or 'L')
bool any_masked(const std::vector<job>& jobs);
// rows of the bands a tile crossing the mask's diagonal is cut into (plan.cpp decompose): each band
// gives at most one ordinary tile (its wholly kept columns) and one edge tile narrower than the
// band is tall, so an edge tile's dense pack op carries fewer than kTriCut dropped columns.
constexpr int kTriCut = 256;
// whether some job of the batch is a scaled one
bool any_scaled(const std::vector<job>& jobs);
// the (A, C) pairs of scaled transforms: FLOAT -> FLOAT, DOUBLE -> DOUBLE, half_pair, fp8_pair
bool scaled_pair(costa_dtype_t src, costa_dtype_t dst);
// whether some job of the batch converts (A's element type differs from C's)
bool any_mixed(const std::vector<job>& jobs);
// whether some job of the batch has a 2-byte element type on either side
bool any_half(const std::vector<job>& jobs);
// whether some job of the batch has a 1-byte element type on either side
bool any_fp8(const std::vector<job>& jobs);
// whether some job of the batch has a packed sub-byte element type on either side
bool any_packed(const std::vector<job>& jobs);

// Build the plan of `rank` (of `n_ranks`) for a batch of jobs (host only).  `loopback` (test
// mode, see loopback_exchange()): 1 = the rank's own tiles all go through pack -> exchange with
// itself -> unpack instead of the local list; 2 = half of them (by a parity of their target
// coordinates, the same on both sides), the rest stays local.
std::unique_ptr<plan> make_plan(const std::vector<job>& jobs, int rank, int n_ranks,
                                int loopback = 0);

// The same plan built on the GPU (device_plan.hip, on `stream` of `device`): identical op lists,
// order and exchange geometry.  nullptr when it does not apply (local blocks that are not exactly
// the rank's grid cells, grids not starting at the same index, more than 2^32 merged cells).
std::unique_ptr<plan> make_plan_device(const std::vector<job>& jobs, int rank, int n_ranks,
                                       int loopback, int device, void* stream);
// planner of plan-cache misses (costa_hip_set_planner, COSTA_PLANNER): 0 host, 1 the GPU for
// layout pairs of at least 4096 blocks, 100000 before the first GPU plan of the process (default),
// 2 the GPU wherever it applies
int planner_mode();
void set_planner_mode(int mode);

// COSTA_LOOPBACK=1 or 2 (test only): a one-rank communicator gets a one-rank RCCL communicator
// and its transforms route tiles through PACK -> ncclSend/ncclRecv to itself -> UNPACK (all of
// them, or half with the rest on the concurrent LOCAL path), so the exchange machinery runs on
// a single GPU (two ranks cannot share one GPU under RCCL).  0 = off.
int loopback_exchange();

// A tuning override `name` from the environment, or nullptr.  Tuning overrides (work-list orders,
// wavefront budgets, shape choices, host-staging slots and threads) are read only when
// COSTA_TUNING=1: a user's environment cannot select shapes and orders that the GPU tests never
// run.  Behaviour switches (COSTA_LOOPBACK, COSTA_MAX_MSG_BYTES, COSTA_EXCHANGE_ROUNDS,
// COSTA_PLANNER, COSTA_HOST_STAGING) and the trace switches are read as documented.
const char* tuning_env(const char* name);

// largest single ncclSend/ncclRecv of the exchange (COSTA_MAX_MSG_BYTES, default 256 MiB)
size_t max_message_bytes();

// parts a peer's package (of at least 16 MiB) is exchanged in, each its own RCCL group, so that
// pack, exchange and unpack overlap (COSTA_EXCHANGE_ROUNDS, default 4; every rank must agree)
int exchange_rounds();
// the threshold in bytes (16 MiB; COSTA_ROUND_MIN_BYTES, a tuning override for the GPU tests)
size_t round_min_bytes();
// element range [lo, hi) of round r of R of a package of n elements of E bytes (one part below the
// threshold; empty at n past its parts)
void round_range(int64_t n, size_t E, int R, int r, int64_t& lo, int64_t& hi);

// normalise one copy_and_transform call (memory_utils.hpp:339-412) into a tile op
costa_tile_op_t make_tile_op(int n_rows, int n_cols, uint64_t src, int src_stride, bool src_cm,
                             uint64_t dst, int dst_stride, bool dst_cm, bool transpose, bool conj,
                             uint32_t scale_kind, uint32_t slot, size_t elem);
// ... of a converting op (source and destination element sizes differ)
costa_tile_op_t make_tile_op(int n_rows, int n_cols, uint64_t src, int src_stride, bool src_cm,
                             uint64_t dst, int dst_stride, bool dst_cm, bool transpose, bool conj,
                             uint32_t scale_kind, uint32_t slot, size_t src_elem, size_t dst_elem);

// scale kind of (alpha, beta) for `dtype` with the reference's branch rules
uint32_t scale_kind(costa_dtype_t dtype, const scal& s, bool copy_mode, bool conj);

// ---- executor (engine.cpp / tile_kernels.hip) ----
int device_count();
int rccl_version();  // ncclGetVersion of the RCCL this process loaded
struct comm;
struct comm* comm_self(int device);
struct comm* comm_create(const unsigned char* id, int nranks, int rank, int device);
// rank emulation (test mode, costa_hip.h): a communicator planned like an RCCL one of that rank and
// size, whose transforms launch one selected part against the caller's package
struct comm* comm_emulated(int rank, int nranks, int device);
void comm_emulate(struct comm* c, int part, int round, void* buffer);
void comm_unique_id(unsigned char* out);
int comm_rank(const struct comm* c);
int comm_size(const struct comm* c);
void comm_destroy(struct comm* c);

// blocking (default) or stream-ordered (async: device-resident layouts only; `user_stream`, a
// hipStream_t or null, is joined at entry and waits for the result)
void transform(const std::vector<job>& jobs, struct comm* c, void* user_stream = nullptr,
               bool async = false);
void synchronize(struct comm* c);  // wait for every queued transform of c's device
void resolve_pending();            // fold finished timing brackets into the statistics
// event time of the edge-tile launches of triangular transforms (profiling on), a part of the
// statistics' local_ms / unpack_ms
double tri_phase_ms(bool reset);

void copy_and_transform(costa_dtype_t dtype, int n_rows, int n_cols, const void* src,
                        int src_stride, bool src_cm, void* dst, int dst_stride, bool dst_cm,
                        bool trans, bool conj, const void* alpha, const void* beta);

void execute_tiles(costa_dtype_t dtype, const costa_tile_op_t* ops, int64_t n,
                   const void* src_base, void* dst_base, const void* scalars, int n_slots,
                   int device);
// a list of converting ops (src_dtype != dst_dtype, a supported pair); scalars in dst_dtype
void execute_tiles_mixed(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* ops,
                         int64_t n, const void* src_base, void* dst_base, const void* scalars,
                         int n_slots, int device);

// ---- the strip kernel families (strip_work.hpp: work lists; strip_launch.hpp: their launch) ----
// the result of their work-list builders: work items, and whether any listed op transposes (the
// others need no LDS tile)
struct strip_list {
    int64_t n_items = 0;
    bool any_transpose = false;
};

// ---- converting lists: dst = g(static_cast<dst type>(src)) ----
// One kernel family per kind of pair, one workgroup per sub-tile of one op; the work items are
// (op index << 32) | sub-tile, as for tile_kernel, in list order.  Scale kind BITCOPY of a
// converting op means "convert only".  The kinds (engine.cpp, pair table): wide_pair -- FLOAT <->
// DOUBLE, CFLOAT <-> CDOUBLE (convert_kernels.hip); half_pair (half_kernels.hip, fp32 scalars:
// dst = cvt(g(w(src), w(dst))), costa_hip.h "Half precision"); fp8_pair (fp8_kernels.hip).
// Each file exports its kind as a pair_family:
struct pair_family {
    bool (*has)(costa_dtype_t src, costa_dtype_t dst);
    // the sub-tile of a pair: elements along the source's fast (*bf) and slow (*bs) dimension
    void (*subtile)(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs);
    void (*launch)(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* d_ops,
                   const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                   const void* d_scalars, void* stream /* hipStream_t */);
};
bool wide_pair(costa_dtype_t src, costa_dtype_t dst);
pair_family wide_family(), half_family(), fp8_family();
// ... and these go to the pair's family (throwing for a pair without one):
bool convertible(costa_dtype_t src, costa_dtype_t dst);  // wide_pair, half_pair or fp8_pair
void convert_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs);
// the work list of a converting list: `ordered` = the ops with each side's VEC flag set from its
// actual address (base + offset) and element size, `work` = every sub-tile of every op
strip_list build_convert_work(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                              const std::vector<costa_tile_op_t>& ops, uint64_t src_base,
                              uint64_t dst_base, std::vector<costa_tile_op_t>& ordered,
                              std::vector<uint64_t>& work);
void launch_convert(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* d_ops,
                    const uint64_t* d_work, const strip_list& l, const char* src_base,
                    char* dst_base, const void* d_scalars, void* stream /* hipStream_t */);

// ---- edge tiles of triangular transforms (tri_kernels.hip) ----
// One kernel family, tri_kernel<T>, one workgroup per sub-tile of one costa_tri_op_t; the work
// items are (op index << 32) | (sub-tile << 1) | whole, `whole` meaning every element of the
// sub-tile is kept.  Sub-tiles without a kept element are not listed.
void tri_subtile(costa_dtype_t dtype, int* bf, int* bs);
// `ordered` = the ops with each side's VEC flag set from its actual address (base + offset)
strip_list build_tri_work(costa_dtype_t dtype, const std::vector<costa_tri_op_t>& ops, uint64_t src_base,
                        uint64_t dst_base, std::vector<costa_tri_op_t>& ordered,
                        std::vector<uint64_t>& work);
void launch_tri(costa_dtype_t dtype, const costa_tri_op_t* d_ops, const uint64_t* d_work,
                const strip_list& l, const char* src_base, char* dst_base, const void* d_scalars,
                void* stream /* hipStream_t */);
void execute_tiles_tri(costa_dtype_t dtype, const costa_tri_op_t* ops, int64_t n, const void* src_base,
                       void* dst_base, const void* scalars, int n_slots, int device);

// ---- scaled transforms (scaled_kernels.hip) ----
// One kernel family, scaled_kernel<Es, Ed>, one workgroup per sub-tile of one costa_scaled_op_t; the
// work items are (op index << 32) | sub-tile.  `row_scale` / `col_scale` are kernel arguments.
void scaled_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs);
// ... of an MX pair (build_scaled_work lists them too) and of a block-scaled pair (build_block_work's
// regions when it quantises, build_scaled_work's sub-tiles when it dequantises)
void mx_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs);
void block_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs);
// `ordered` = the ops with each side's VEC flag set from its actual address (base + offset) and its
// strip's alignment, `work` = every sub-tile of every op: in list order, or (dst_order) by the
// address of the sub-tile's first destination element
strip_list build_scaled_work(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                             const std::vector<costa_scaled_op_t>& ops, uint64_t src_base,
                             uint64_t dst_base, std::vector<costa_scaled_op_t>& ordered,
                             std::vector<uint64_t>& work, bool dst_order);
// (row_amax / col_amax: the amax outputs, device arrays of the compute type's unsigned integer; with
// one of them the list runs on the AMAX instantiation, with neither on today's kernels)
void launch_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* d_ops,
                   const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                   const void* d_scalars, const void* row_scale, const void* col_scale, void* row_amax,
                   void* col_amax, void* stream /* hipStream_t */);
void execute_tiles_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                          int64_t n, const void* src_base, void* dst_base, const void* scalars,
                          int n_slots, const void* row_scale, const void* col_scale, int device);
// sub-tiles run by scaled_kernel since the last reset
int64_t scaled_items(bool reset);
// ---- amax outputs (costa_hip.h, "amax outputs") ----
// costa_hip_execute_tiles_scaled plus the two outputs; the scales may both be null
void execute_tiles_amax(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                        int64_t n, const void* src_base, void* dst_base, const void* scalars,
                        int n_slots, const void* row_scale, const void* col_scale, void* row_amax,
                        void* col_amax, int device);
// the element types costa_hip_layout_amax reduces: FLOAT, DOUBLE, the 2-byte and the 1-byte types
bool amax_dtype(costa_dtype_t t);
// one source-only op per local block of L (host only): src = the block's address, nf x ns its extent
// along its fast and slow index, (row0, col0) from the first row / column of L's matrix,
// COSTA_SCALED_F_ROWS where the fast index walks rows (ordering 'C')
std::vector<costa_scaled_op_t> layout_amax_ops(const elayout& L);
// the reduce-only kernel (amax_kernel<Es>) over such ops and their work items (build_scaled_work)
void launch_amax(costa_dtype_t dtype, const costa_scaled_op_t* d_ops, const uint64_t* d_work,
                 int64_t n_items, void* row_amax, void* col_amax, void* stream /* hipStream_t */);
void layout_amax(const elayout& L, void* row_amax, void* col_amax, struct comm* c, void* user_stream,
                 bool async);
// sub-tiles run by the AMAX instantiations of scaled_kernel and by amax_kernel since the last reset
int64_t amax_items(bool reset);
// ---- MX block-scaled transforms (mx_kernels.hip; costa_hip.h, "MX block-scaled transforms") ----
// One kernel family, mx_kernel<Es, Ed, QUANT, SR>, on the scaled ops and work items of a scaled plan
// (build_scaled_work: the same 64 x 64 sub-tile and alignment rule).  A scale tensor as the kernel
// sees it, in TARGET coordinates (C's; A's descriptor has its axis turned round when the job
// transposes): byte of (block b, line l) at data[b * block_stride + l * line_stride], `rows` = a
// block is 32 consecutive target rows of one target column.  data == nullptr: none.
struct mx_side {
    void* data = nullptr;
    int64_t block_stride = 0, line_stride = 0;
    bool rows = true;
};
// FLOAT -> Q (quantise), Q -> FLOAT (dequantise), Q -> Q of one Q (requantise); Q an FP8 type,
// COSTA_FP4_E2M1 or an FP6 type
bool mx_pair(costa_dtype_t src, costa_dtype_t dst);
// the per-op half of the evenness rule ("FP4 pair") and of the quad rule ("FP6 quad") on caller-given
// ops: on each packed side the leading dimension and the extent along the side's stored-contiguous
// dimension are multiples of the packing group
void check_packed_ops(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const std::vector<costa_scaled_op_t>& ops);
// Stochastic rounding (costa_hip.h, "Stochastic rounding in the MX transforms"): the two 32-bit keys
// of a call's seed, which the SR instances mx_kernel<.., QUANT, SR> take as kernel arguments, and the
// 24 random bits of target element (i, j) (host only; the kernels compute the same)
struct mx_sr {
    uint32_t k0 = 0, k1 = 0;
};
mx_sr mx_sr_keys(uint64_t seed);
uint32_t mx_sr_bits(uint64_t seed, int64_t i, int64_t j);
// a scale tensor on exactly the FP8 sides of the pair; `ceil`: COSTA_MX_CEIL; `sr` (quantising pairs
// only): the SR instance with these keys, nullptr: round to nearest even
void launch_mx(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* d_ops,
               const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
               const void* d_scalars, const mx_side& a_scales, const mx_side& c_scales, bool ceil,
               void* stream /* hipStream_t */, const mx_sr* sr = nullptr);
// a descriptor's strides are positive and no two (block, line) of a rows x cols matrix share a byte
// (throws COSTA_ERR_ARG naming `what`); host only
void check_mx_scales(const costa_mx_scales_t& s, int64_t rows, int64_t cols, const std::string& what);
// the tile-boundary rule: along `axis` every op starts at a multiple of 32 of C's coordinates and
// spans a multiple of 32 or ends at the edge of C's m x n matrix (throws COSTA_ERR_ARG, "MX block")
void check_mx_ops(const std::vector<costa_scaled_op_t>& ops, int axis, int64_t m, int64_t n);
// costa_hip_execute_tiles_mx: m x n is C's matrix; a_transposed: A's matrix is n x m (target (i, j)
// is A's (j, i))
// `seed` (costa_hip_execute_tiles_mx_sr): stochastic rounding with this seed, a quantising pair only
void execute_tiles_mx(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                      int64_t n_ops, const void* src_base, void* dst_base, const void* scalars, int n_slots,
                      const costa_mx_scales_t* a_scales, const costa_mx_scales_t* c_scales, int rounding,
                      int64_t m, int64_t n, int a_transposed, int device, const uint64_t* seed = nullptr);
// sub-tiles run by mx_kernel since the last reset
int64_t mx_items(bool reset);
// ---- dual-output MX quantise (mx_dual_kernels.hip; costa_hip.h, "Dual-output MX quantise") ----
// mx_dual_kernel<Ed, SR> on costa_dual_op_t: FLOAT -> Q into output 1 (the scaled op) and, from the same
// load, into output 2 (dst2 / ldd2 / flags2), whose element has target coordinates (j, i).
// The work list: build_scaled_work's rule for output 1's sides, the same alignment rule for output 2's
// VEC_DST at its own address; any_transpose where either output transposes
strip_list build_dual_work(costa_dtype_t dst_dtype, const std::vector<costa_dual_op_t>& ops, uint64_t src_base,
                           uint64_t dst_base, uint64_t dst2_base, std::vector<costa_dual_op_t>& ordered,
                           std::vector<uint64_t>& work, bool dst_order);
// c_scales in C's coordinates, ct_scales in Ct's (both required)
void launch_mx_dual(costa_dtype_t dst_dtype, const costa_dual_op_t* d_ops, const uint64_t* d_work,
                    const strip_list& l, const char* src_base, char* dst_base, char* dst2_base,
                    const void* d_scalars, const mx_side& c_scales, const mx_side& ct_scales, bool ceil,
                    void* stream /* hipStream_t */, const mx_sr* sr = nullptr);
// output 2's op as a scaled op of its own n x m matrix (row0 / col0 swapped, F_ROWS complemented, its
// address, leading dimension and store mode): what the per-op rules are checked on
costa_scaled_op_t dual_twin_op(const costa_dual_op_t& t);
// the twin of every op: rows [c0, c1) x columns [r0, r1) of Ct lie inside one block of Ct that is
// local to `rank` (throws COSTA_ERR_ARG, "dual layouts", with the rectangle)
std::vector<costa_dual_op_t> dual_twins(const std::vector<costa_scaled_op_t>& ops, const elayout& Ct, int rank);
// the per-op rules of both outputs on dual ops: "MX block" along each output's axis (axis < 0: not
// checked; the message names the output), the packed rules on both destinations
void check_dual_ops(costa_dtype_t dst_dtype, const std::vector<costa_dual_op_t>& ops, int c_axis, int ct_axis,
                    int64_t m, int64_t n);
// costa_hip_execute_tiles_mx_dual: m x n is output 1's matrix
void execute_tiles_mx_dual(costa_dtype_t dst_dtype, const costa_dual_op_t* ops, int64_t n_ops, const void* src_base,
                           void* dst_base, void* dst2_base, const void* scalars, int n_slots,
                           const costa_mx_scales_t* c_scales, const costa_mx_scales_t* ct_scales, int rounding,
                           int64_t m, int64_t n, const uint64_t* seed, int device);
// sub-tiles run by mx_dual_kernel since the last reset (mx_items does not count them)
int64_t mx_dual_items(bool reset);
// ---- block-scaled FP8 transforms (block_kernels.hip; costa_hip.h, "Block-scaled FP8 transforms") ----
// block_kernel<Es, Ed, QUANT> on the scaled ops of a scaled plan: dequantising lists run the plan's
// 64 x 64 work items (build_scaled_work), quantising ones 128 x 128 regions (build_block_work, whose
// `ordered` equals build_scaled_work's: the same ops, order and VEC flags).  A scale tensor as the
// kernel sees it, in TARGET coordinates (A's descriptor has rows and columns swapped when the job
// transposes): the float of target (i, j) at data[(i >> row_shift) * row_stride + (j >> col_shift) *
// col_stride], a shift 0 or 7.  data == nullptr: none.
struct block_side {
    void* data = nullptr;
    int64_t row_stride = 0, col_stride = 0;
    int32_t row_shift = 0, col_shift = 0;
};
// FLOAT -> Q (quantise), Q -> FLOAT (dequantise), Q -> Q of one Q (requantise); Q an FP8 type
bool block_pair(costa_dtype_t src, costa_dtype_t dst);
strip_list build_block_work(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                            const std::vector<costa_scaled_op_t>& ops, uint64_t src_base, uint64_t dst_base,
                            std::vector<costa_scaled_op_t>& ordered, std::vector<uint64_t>& work, bool dst_order);
// a scale tensor on exactly the FP8 sides of the pair; `d_work` / `l`: regions when c_scales is
// given, sub-tiles otherwise; `pow2`: COSTA_BLOCK_POW2
void launch_block(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* d_ops,
                  const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                  const void* d_scalars, const block_side& a_scales, const block_side& c_scales, bool pow2,
                  void* stream /* hipStream_t */);
// a descriptor's block shape is (1, 128), (128, 1) or (128, 128), data is 4-byte aligned, the strides
// are positive and no two blocks of a rows x cols matrix share a float (throws COSTA_ERR_ARG naming
// `what`); host only
void check_block_scales(const costa_block_scales_t& s, int64_t rows, int64_t cols, const std::string& what);
// the tile-boundary rule: every op starts at a multiple of the block shape in C's coordinates and
// spans a multiple of it or ends at the edge of C's m x n matrix (throws COSTA_ERR_ARG, "scale block")
void check_block_ops(const std::vector<costa_scaled_op_t>& ops, int block_rows, int block_cols, int64_t m,
                     int64_t n);
// costa_hip_execute_tiles_block_scaled: as execute_tiles_mx
void execute_tiles_block(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                         int64_t n_ops, const void* src_base, void* dst_base, const void* scalars, int n_slots,
                         const costa_block_scales_t* a_scales, const costa_block_scales_t* c_scales,
                         int rounding, int64_t m, int64_t n, int a_transposed, int device);
// work items (sub-tiles and regions) run by block_kernel since the last reset
int64_t block_items(bool reset);
// ... of every scaled unpack op (plan::unpack_scaled), by the rule of exchange_round_of_ops
void exchange_round_of_scaled(const struct plan& p, int rounds, std::vector<int>& unpack_round);

// kernel launcher (tile_kernels.hip); `work` and `ops` are device arrays
// ops small enough for one wavefront each (tiny path): copy mode up to kTinyCopyBytes of
// data, transpose mode up to kTinyLdsBytes of staged tile (row pitch nf | 1); the defaults
// are smaller (tiny_copy_budget: one pass of the wavefront; kTinyLdsDefault staged)
constexpr int kTinyCopyBytes = 16384;
constexpr int kTinyLdsBytes = 8192;
// r11, cfg 5 'T' with the XCD remap and 32 bytes per lane per pass: 3.80 TB/s at 4 KiB
// against 3.0 at 8 KiB (profiles/r11/tiny_variants*.log)
constexpr int kTinyLdsDefault = 4096;
// staged bytes of one transposing wavefront op (kTinyLdsDefault);
// the launch gives each wavefront that much LDS
int64_t tiny_lds_budget();
// bytes a lane of the wavefront copy path moves per pass (tile_kernels.hip tiny_copy_bytes)
// (64 for every type since r11: 4-byte types at 128 gave cfg 5 'N' 3.77 against 4.15 TB/s once
// the XCD remap was on, profiles/r11/c5_budget.log; fewer VGPRs, more resident wavefronts)
constexpr int tiny_copy_lane_bytes(size_t) { return 64; }
// bytes of one copy-mode wavefront op / of one transposing wavefront op's staged tile (the
// budgets the host split cuts to)
int64_t tiny_copy_budget(int64_t elem_size, bool local_list = true);
// a large op that is not 16-byte aligned on both sides takes the wavefront path up to this many
// large sub-tiles of data (engine.cpp wave_knobs::policy)
constexpr int64_t kUnalignedWaveCap = 4;
constexpr int tiny_lds_bytes = kTinyLdsBytes;

struct launch_args {
    const costa_tile_op_t* ops;  // device, in build_work order: [sub-tiled ops | tiny ops]
    const uint64_t* work;   // per sub-tile: (op index << 32) | sub-tile index
    int64_t n_large;        // work items using the large sub-tile shape
    int64_t n_medium;       // then work[n_large, n_large + n_medium): the medium shape
    int64_t n_skew = 0;     // then n_skew items of the skew shape (unaligned destinations)
    int64_t n_cblock = 0;   // then n_cblock destination-block groups: index of the group's header op
    int64_t cblock_lds = 0; // LDS image of the largest group (elements)
    int cb_map = 0;         // cblock_map of the groups
    int64_t tiny_first;     // ops[tiny_first, tiny_first + n_tiny) run one per wavefront
    int64_t n_tiny;
    const char* src_base;
    char* dst_base;
    const void* scalars;    // device: n_slots x (alpha, beta) of the dtype
    bool any_transpose;     // false: copy-mode ops only, launch without the LDS tile
    bool any_axpby;         // false: no op reads its destination (beta == 0 everywhere)
    bool tr_shape;          // the work items are sub-tiles of the transposing lists' shape
    bool sq;                // ... of its square variant (work_split::sq)
    bool full;              // work_split::full
    bool med_full;          // work_split::med_full
    bool med_sq;            // work_split::med_sq
    bool skew_wide = false; // work_split::skew_wide
};
bool any_transpose(const std::vector<costa_tile_op_t>& ops);
bool any_axpby(const std::vector<costa_tile_op_t>& ops);
void launch_tiles(costa_dtype_t dtype, const launch_args& a, void* stream /* hipStream_t */);
// the wavefront pieces of a list with destination-block groups run as workgroups after the groups
// in the group kernel's launch (its tail) instead of a tiny_kernel launch (COSTA_FUSE_PIECES)
bool pieces_in_group_launch(int64_t n_cblock, int64_t n_tiny);
// destination columns taller than this are walked in panels of this many bytes of rows (engine.cpp
// build_work)
constexpr int64_t kPanelBytes = int64_t(128) << 10;
// destination-block groups (tile_kernels.hip cblock_kernel): threads per workgroup and 16-byte
// destination vectors per thread; a group holds at most kCblockThreads * kCblockChunks vectors
constexpr int kCblockThreads = 256;
constexpr int kCblockChunks = 4;
inline int64_t cblock_max_elems(int64_t E) { return int64_t(kCblockThreads) * kCblockChunks * (16 / E); }
// work-list position of workgroup b of a launch of nb destination-block groups of a transposing
// list (tile_kernels.hip cblock_kernel): the hardware deals workgroups round-robin over the 8
// XCDs; chunks of kCblockXcdChunk consecutive groups go to one XCD, the 8 XCDs on 8 adjacent
// chunks; the last partial round of chunks keeps the plain order.  A permutation of [0, nb)
// (tools/work_check.cpp xcd).  (constexpr: host and device.)
// r6: 16 (traffic of cfg 5 'T' 1.134x -> 1.050x of its algorithmic bytes; chunks of 4 / 8 / 12 /
// 16 in-run 0.600 / 0.602 / 0.605 / 0.605 ms, rocprofv3 590.7 / 591.4 / 589.5 / 595.5 us;
// profiles/r6m/, r6n/)
constexpr int64_t kCblockXcdChunk = 16;
constexpr int64_t cblock_xcd_order(int64_t b, int64_t nb, int64_t ch = kCblockXcdChunk) {
    return b / (8 * ch) * (8 * ch) + 8 * ch <= nb ? b / (8 * ch) * (8 * ch) + (b % 8) * ch + (b / 8) % ch : b;
}
// work-list position of workgroup b of nb when XCD x (= b mod 8) walks the x-th of 8 contiguous
// slices of the list, slice x holding nb / 8 items (one more for the first nb mod 8 slices).  A
// permutation of [0, nb); tiny_kernel's remap and the destination-block groups' XCD column bands
// (engine.cpp cblock_groups).  (constexpr: host and device.)
constexpr int64_t xcd_slice_order(int64_t b, int64_t nb) {
    return (b % 8) < nb % 8 ? (b % 8) * (nb / 8 + 1) + b / 8
                            : (nb % 8) * (nb / 8 + 1) + ((b % 8) - nb % 8) * (nb / 8) + b / 8;
}
// how a launch of destination-block groups maps workgroups onto the list (work_split::cb_map)
enum cblock_map { cb_round_robin = 0, cb_xcd_chunks = 1, cb_xcd_bands = 2 };
// sub-tile shapes (elements along the source's fast dim, along its slow dim) of a copy-only list
// or of a list with transposing ops: the large shape, the medium one (bf_m = bs_m = 0: none) and
// the large shape's square variant for lists whose large ops all fit it (bf_q = bs_q = 0: none),
// and the 32 x 32 shape the medium class takes when its ops all fit it (bf_s x bs_s)
struct shape_dims {
    int bf = 0, bs = 0, bf_m = 0, bs_m = 0, bf_q = 0, bs_q = 0, bf_s = 0, bs_s = 0;
    int cf = 0, cs = 0;  // the large class's dimensions (classification, merging): bf x bs for
                         // transposing lists, the r4 copy sub-tile for copy-only lists
    int bf_k = 0, bs_k = 0;  // the skew shape (transposes into unaligned destinations; 0: none)
    int bf_kw = 0, bs_kw = 0;  // its wide variant (sources off the 16-byte grid too; 4-byte types)
};
void tile_shapes(costa_dtype_t dtype, bool transposing_list, shape_dims* out);
// Execution order of an op list: `ordered` = [sub-tiled ops | tiny ops] (tiny ops sorted by the
// planner's locality hint, so wavefronts running at the same time share partially used cache
// lines),
// `work` = [large-shape sub-tiles | small-shape sub-tiles], indices into `ordered`.
struct work_split {
    int64_t n_large = 0, n_medium = 0, tiny_first = 0, n_tiny = 0;
    int64_t n_skew = 0;     // skew-shape work items, after the medium ones
    int64_t n_cblock = 0;   // destination-block groups, after the skew items (cblock_groups)
    int64_t cblock_lds = 0; // elements of the largest group's LDS image
    int cb_map = 0;         // cblock_map: how the groups' launch maps workgroups onto them
    bool tr_shape = false;  // sub-tiles cut with tile_shapes(dtype, true, ...)
    bool sq = false;        // ... the large ops with its square variant (bf_q x bs_q)
    bool full = false;      // every large op of a transposing list is aligned and a whole number
                            // of large sub-tiles (the launch may then take fewer threads)
    bool med_full = false;  // the same for the medium ops and the medium sub-tile
    bool med_sq = false;    // the medium class runs on 32 x 32 sub-tiles (bf_s x bs_s)
    bool skew_wide = false; // the skew items are sub-tiles of its wide variant (bf_kw x bs_kw)
    int64_t n_items() const { return n_large + n_medium + n_skew + n_cblock + n_tiny; }
};
// list_pack: the ops write the dense send package (their destinations are contiguous whatever
// their order), which changes the wavefront ops' order (wave_knobs::sort); local lists (both
// sides user matrices) cut copy ops finer than pack / unpack lists (tiny_copy_budget)
enum list_kind { list_local, list_pack, list_unpack };
// The part of a work list that build_work left on the GPU: the destination-block groups built by
// device_lists.hip.  `ordered` entries [at_ordered, at_ordered + n_ordered) and `work` entries
// [at_work, at_work + n_work) are d_ordered / d_work; the host vectors hold all the others, without
// a gap.  A caller that passes one (device, stream set) lets build_work build the groups there
// (list_builder_mode; `force`: wherever it applies).
struct device_section {
    int device = -1;
    void* stream = nullptr;  // hipStream_t
    bool force = false;
    std::shared_ptr<void> mem;  // owns d_ordered and d_work
    costa_tile_op_t* d_ordered = nullptr;
    uint64_t* d_work = nullptr;
    size_t at_ordered = 0, n_ordered = 0, at_work = 0, n_work = 0;
};
work_split build_work(costa_dtype_t dtype, const std::vector<costa_tile_op_t>& ops,
                      std::vector<costa_tile_op_t>& ordered, std::vector<uint64_t>& work,
                      list_kind kind = list_local, device_section* dev = nullptr, bool dst_order = false);
// (dst_order: the shaped sub-tiles in destination-address order whatever the ops do -- the ordinary
// LOCAL list of a triangular plan, engine.cpp get_plan)
// builder of the destination-block groups on a plan-cache miss (costa_hip_set_list_builder,
// COSTA_LIST_BUILDER): 0 the host, 1 the GPU for lists of at least kDeviceGroupsMin wavefront ops
// (default), 2 the GPU wherever it applies
constexpr size_t kDeviceGroupsMin = 16384;
int list_builder_mode();
void set_list_builder_mode(int mode);
// engine.cpp cblock_groups on the GPU (device_lists.hip): the same groups in the same order, the
// same bytes.  `wave`: the wavefront ops as indices into `ops`, in list order; base_at: the size of
// `ordered` so far (header indices count from there).  Fills sec's device part and `taken` (per
// wavefront op: it joined a group); -> the number of groups, or -1 when the GPU declines (keys
// wider than 64 bits) and the host builder must run.
int64_t cblock_groups_device(int64_t E, int64_t budget, uint32_t vec_bits, int bands_env,
                             const std::vector<costa_tile_op_t>& ops, const std::vector<uint32_t>& wave,
                             size_t base_at, device_section& sec, std::vector<char>& taken,
                             int64_t& lds, int& map);
// one list's work lists, built on the host (device < 0) or with the groups on GPU `device`, copied
// out whole (costa_hip_work_export); -> whether the GPU built part of them
bool work_export(costa_dtype_t dtype, const std::vector<costa_tile_op_t>& ops, list_kind kind,
                 int device, std::vector<costa_tile_op_t>& ordered, std::vector<uint64_t>& work,
                 work_split& w);
// launch arguments of one ordered op list
launch_args make_launch(const work_split& w, const void* d_ordered, const void* d_work,
                        const char* src_base, char* dst_base, const void* d_scalars, bool transpose,
                        bool axpby);

// ---- host-resident pipeline (host_pipe.cpp) ----
// Transforms whose layouts all live in host memory: pack, local and unpack ops in groups of
// dense packages moving through a pinned/device slot ring (H2D, kernels, the exchange and D2H
// overlap).
struct host_pipeline;
// false when a pack op's column exceeds a pipeline slot (the mirror scheme is used then)
bool host_pipeline_accepts(costa_dtype_t dtype, const std::vector<costa_tile_op_t>& pack_ops);
// pack_round / unpack_round: each op's exchange round (exchange_round_of_ops) of `rounds`
std::shared_ptr<host_pipeline> make_host_pipeline(costa_dtype_t dtype,
                                                  const std::vector<costa_tile_op_t>& pack_ops,
                                                  const std::vector<costa_tile_op_t>& local_ops,
                                                  const std::vector<costa_tile_op_t>& unpack_ops,
                                                  const std::vector<int>& pack_round,
                                                  const std::vector<int>& unpack_round, int rounds);
size_t host_pipeline_groups(const host_pipeline& hp);
// Blocking: returns when every target byte is back in host memory.  Tile kernels run on
// `compute_stream`; `exchange(stream, r)` (empty without one) is called once per round r, with
// `exchange_stream`, when round r's part of the send package is in `send_buf`; the unpack
// kernels of round r read `recv_buf` after it.
void run_host_pipeline(host_pipeline& hp, int device, void* compute_stream, void* exchange_stream,
                       char* send_buf, char* recv_buf,
                       const std::function<void(void*, int)>& exchange, const void* d_scalars);
// the exchange round of every pack op (by its first element) and unpack op (by its last)
void exchange_round_of_ops(const struct plan& p, int rounds, std::vector<int>& pack_round,
                           std::vector<int>& unpack_round);
// ... of every edge unpack op (plan::unpack_tri), by the same rule
void exchange_round_of_tri(const struct plan& p, int rounds, std::vector<int>& unpack_tri_round);
void release_host_rings();
// host staging of host-resident layouts: 0 = mirror (every spanned range up, kernels, target
// ranges down), 1 = pipelined (default; falls back to the mirror where it does not apply)
int host_staging_mode();
void set_host_staging_mode(int mode);

// errors
struct error : std::runtime_error {
    int code;
    error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// statistics
costa_stats_t& stats();
bool profiling();
void set_profiling(bool on);
void release_caches();

}  // namespace engine
}  // namespace costa
