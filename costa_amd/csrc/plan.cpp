// Tile planner: turns (A layout, C layout, op, alpha, beta) into the pack / local / unpack
// tile-op lists of one rank.
//
// Reference algorithm followed (eth-cscs/COSTA):
//   transform(): transpose A's view when op != 'N'        grid2grid/transform.cpp:162-200
//   decompose_blocks / decompose_block                     grid2grid/utils.hpp:26-115
//     cover of a block by the other grid                   grid2grid/grid_cover.cpp:54-121
//     sub-tile pointer (stored orientation)                grid2grid/block.cpp:72-111
//   message sort key (peer, tag, rows, cols, |a|,|b|,...)  communication_data.cpp:67-82,
//                                                          block.cpp:121-125
//   communication_data: local vs remote split, running     communication_data.cpp:103-164
//     offsets, per-peer counts, displacements
//   copy_to_buffer / copy_from_buffer / copy_local_blocks  communication_data.cpp:191-302
//     -> copy_and_transform normalisation                  memory_utils.hpp:330-412
// The cover is found by binary search instead of the reference's merged linear scan;
// the resulting tile set and order are identical.
#include "engine.hpp"
#include "tile_op.hpp"

#include <algorithm>
#include <cctype>
#include <complex>
#include <cstring>
#include <exception>
#include <string>
#include <thread>

namespace costa {
namespace engine {

size_t dtype_size(costa_dtype_t t) {
    switch (t) {
    case COSTA_FLOAT: return 4;
    case COSTA_DOUBLE: return 8;
    case COSTA_CFLOAT: return 8;
    case COSTA_CDOUBLE: return 16;
    case COSTA_INT32: return 4;
    case COSTA_HALF: return 2;
    case COSTA_BFLOAT16: return 2;
    case COSTA_FP8_E4M3: return 1;
    case COSTA_FP8_E5M2: return 1;
    // (half a byte: elem_size() says it; whoever asks for whole bytes does not take the type)
    case COSTA_FP4_E2M1:
        throw error(COSTA_ERR_ARG, "costa: FP4_E2M1 elements are half a byte: only the MX entry points "
                                   "(costa_hip_transform_mx, costa_hip_execute_tiles_mx) take them");
    // (three quarters of a byte)
    case COSTA_FP6_E2M3:
    case COSTA_FP6_E3M2:
        throw error(COSTA_ERR_ARG, std::string("costa: ") + dtype_name(t) +
                                       " elements are three quarters of a byte: only the MX entry points "
                                       "(costa_hip_transform_mx, costa_hip_execute_tiles_mx) take them");
    }
    throw error(COSTA_ERR_ARG, "unknown dtype");
}

esize elem_size(costa_dtype_t t) {
    return dtype_is_fp4(t) ? esize::packed(4) : dtype_is_fp6(t) ? esize::packed(6) : esize(dtype_size(t));
}
size_t pkg_unit_size(costa_dtype_t pkg) { return dtype_is_packed(pkg) ? 1 : dtype_size(pkg); }
int64_t pkg_units(costa_dtype_t pkg, int64_t elems) {
    return dtype_is_packed(pkg) ? int64_t(elem_size(pkg).bytes(uint64_t(elems))) : elems;
}

bool dtype_is_complex(costa_dtype_t t) { return t == COSTA_CFLOAT || t == COSTA_CDOUBLE; }
bool dtype_is_half(costa_dtype_t t) { return t == COSTA_HALF || t == COSTA_BFLOAT16; }

bool dtype_is_fp8(costa_dtype_t t) { return t == COSTA_FP8_E4M3 || t == COSTA_FP8_E5M2; }
bool dtype_is_fp4(costa_dtype_t t) { return t == COSTA_FP4_E2M1; }
bool dtype_is_fp6(costa_dtype_t t) { return t == COSTA_FP6_E2M3 || t == COSTA_FP6_E3M2; }
int packed_group(costa_dtype_t t) { return dtype_is_fp4(t) ? 2 : dtype_is_fp6(t) ? 4 : 0; }
bool dtype_is_packed(costa_dtype_t t) { return packed_group(t) != 0; }
const char* packed_rule(costa_dtype_t t) { return dtype_is_fp6(t) ? "FP6 quad" : "FP4 pair"; }

costa_dtype_t compute_dtype(costa_dtype_t src, costa_dtype_t dst) {
    return dtype_is_half(src) || dtype_is_half(dst) || dtype_is_fp8(src) || dtype_is_fp8(dst) ||
                   dtype_is_packed(src) || dtype_is_packed(dst)
               ? COSTA_FLOAT
               : dst;
}

bool half_pair(costa_dtype_t src, costa_dtype_t dst) {
    return (dtype_is_half(src) && (dst == src || dst == COSTA_FLOAT)) ||
           (src == COSTA_FLOAT && dtype_is_half(dst));
}

bool fp8_pair(costa_dtype_t src, costa_dtype_t dst) {
    return (dtype_is_fp8(src) && (dst == src || dst == COSTA_FLOAT)) ||
           (src == COSTA_FLOAT && dtype_is_fp8(dst));
}

bool packed_pair(costa_dtype_t src, costa_dtype_t dst) {
    return (dtype_is_packed(src) && (dst == src || dst == COSTA_FLOAT)) ||
           (src == COSTA_FLOAT && dtype_is_packed(dst));
}

bool wide_pair(costa_dtype_t src, costa_dtype_t dst) {
    return (src == COSTA_FLOAT && dst == COSTA_DOUBLE) || (src == COSTA_DOUBLE && dst == COSTA_FLOAT) ||
           (src == COSTA_CFLOAT && dst == COSTA_CDOUBLE) || (src == COSTA_CDOUBLE && dst == COSTA_CFLOAT);
}

bool convertible(costa_dtype_t src, costa_dtype_t dst) {
    return half_pair(src, dst) || fp8_pair(src, dst) || wide_pair(src, dst);
}

const char* dtype_name(costa_dtype_t t) {
    switch (t) {
    case COSTA_FLOAT: return "FLOAT";
    case COSTA_DOUBLE: return "DOUBLE";
    case COSTA_CFLOAT: return "CFLOAT";
    case COSTA_CDOUBLE: return "CDOUBLE";
    case COSTA_INT32: return "INT32";
    case COSTA_HALF: return "HALF";
    case COSTA_BFLOAT16: return "BFLOAT16";
    case COSTA_FP8_E4M3: return "FP8_E4M3";
    case COSTA_FP8_E5M2: return "FP8_E5M2";
    case COSTA_FP4_E2M1: return "FP4_E2M1";
    case COSTA_FP6_E2M3: return "FP6_E2M3";
    case COSTA_FP6_E3M2: return "FP6_E3M2";
    }
    return "unknown";
}

costa_dtype_t plan_pkg_dtype(costa_dtype_t src, costa_dtype_t dst) {
    if (fp8_pair(src, dst) || packed_pair(src, dst)) return src;
    return dtype_size(src) < dtype_size(dst) ? src : dst;
}

bool any_masked(const std::vector<job>& jobs) {
    for (const job& jb : jobs)
        if (jb.uplo != 'A') return true;
    return false;
}

bool any_scaled(const std::vector<job>& jobs) {
    for (const job& jb : jobs)
        if (jb.scaled) return true;
    return false;
}

bool scaled_pair(costa_dtype_t src, costa_dtype_t dst) {
    return (src == dst && (src == COSTA_FLOAT || src == COSTA_DOUBLE)) || half_pair(src, dst) ||
           fp8_pair(src, dst);
}

bool any_mixed(const std::vector<job>& jobs) {
    for (const job& jb : jobs)
        if (jb.A && jb.C && jb.A->dtype != jb.C->dtype) return true;
    return false;
}

bool any_half(const std::vector<job>& jobs) {
    for (const job& jb : jobs)
        if (jb.A && jb.C && (dtype_is_half(jb.A->dtype) || dtype_is_half(jb.C->dtype))) return true;
    return false;
}

bool any_packed(const std::vector<job>& jobs) {
    for (const job& jb : jobs)
        if (jb.A && jb.C && (dtype_is_packed(jb.A->dtype) || dtype_is_packed(jb.C->dtype))) return true;
    return false;
}

bool any_fp8(const std::vector<job>& jobs) {
    for (const job& jb : jobs)
        if (jb.A && jb.C && (dtype_is_fp8(jb.A->dtype) || dtype_is_fp8(jb.C->dtype))) return true;
    return false;
}

template <> costa_dtype_t dtype_of<float>() { return COSTA_FLOAT; }
template <> costa_dtype_t dtype_of<double>() { return COSTA_DOUBLE; }
template <> costa_dtype_t dtype_of<std::complex<float>>() { return COSTA_CFLOAT; }
template <> costa_dtype_t dtype_of<std::complex<double>>() { return COSTA_CDOUBLE; }
template <> costa_dtype_t dtype_of<int>() { return COSTA_INT32; }
template <> costa_dtype_t dtype_of<half_bits>() { return COSTA_HALF; }
template <> costa_dtype_t dtype_of<bfloat16_bits>() { return COSTA_BFLOAT16; }
template <> costa_dtype_t dtype_of<fp8_e4m3_bits>() { return COSTA_FP8_E4M3; }
template <> costa_dtype_t dtype_of<fp8_e5m2_bits>() { return COSTA_FP8_E5M2; }

template <typename T>
elayout erase(const grid_layout<T>& L) {
    elayout e;
    e.dtype = dtype_of<T>();
    const auto& g = L.grid;
    if (g.is_transposed())
        throw error(COSTA_ERR_ARG, "costa: layouts must not be left transposed by the caller");
    e.rows_split = g.grid().rows_split;
    e.cols_split = g.grid().cols_split;
    e.owners = g.reordered_owners_row_major();  // with a rank relabelling applied
    e.n_ranks = g.num_ranks();
    e.ordering = L.ordering;
    e.blocks.reserve(size_t(L.blocks.num_blocks()));
    for (int i = 0; i < L.blocks.num_blocks(); ++i) {
        const auto& b = L.blocks.get_block(i);
        if (b.transposed)
            throw error(COSTA_ERR_ARG, "costa: layouts must not be left transposed by the caller");
        e.blocks.push_back({b.rows_interval, b.cols_interval,
                            reinterpret_cast<char*>(const_cast<T*>(b.data)), b.stride});
    }
    return e;
}
template elayout erase<float>(const grid_layout<float>&);
template elayout erase<double>(const grid_layout<double>&);
template elayout erase<std::complex<float>>(const grid_layout<std::complex<float>>&);
template elayout erase<std::complex<double>>(const grid_layout<std::complex<double>>&);
template elayout erase<int>(const grid_layout<int>&);
template elayout erase<half_bits>(const grid_layout<half_bits>&);
template elayout erase<bfloat16_bits>(const grid_layout<bfloat16_bits>&);
template elayout erase<fp8_e4m3_bits>(const grid_layout<fp8_e4m3_bits>&);
template elayout erase<fp8_e5m2_bits>(const grid_layout<fp8_e5m2_bits>&);

namespace {

// ---- scalar predicates evaluated exactly as the reference does, in T's arithmetic ----
template <typename T>
T load(const std::array<unsigned char, 16>& b) {
    T v;
    std::memcpy(&v, b.data(), sizeof(T));
    return v;
}

template <typename T>
uint32_t kind_t(const scal& s, bool copy_mode, bool conj) {
    const T a = load<T>(s.alpha), b = load<T>(s.beta);
    // memcpy fast path of memory::copy (memory_utils.hpp:29-33): copy mode only
    if (copy_mode && !conj && !(std::abs(a - T{1}) > 0 || std::abs(b - T{0}) > 0))
        return COSTA_SCALE_BITCOPY;
    if (a == T{0} && b == T{0}) return COSTA_SCALE_ZERO;  // memory_utils.hpp:42-43
    if (b == T{0}) return COSTA_SCALE_ALPHA;               // :44-45
    return COSTA_SCALE_AXPBY;                              // :46-47
}

struct side_tile {
    int peer, tag;
    interval rows, cols;  // target (C) coordinates
    char* ptr;            // first element, stored orientation
    int ld;
    int n_rows, n_cols;   // stored orientation
    bool edge;            // the mask's diagonal cuts it (triangular transforms)
};

// the mask of a triangular transform in target coordinates: element (r, c) is kept when
// (c - oc) - (r - orow) >= k (upper) or <= k (lower); `on` false: no mask
struct tri_mask {
    bool on = false, upper = true;
    int k = 0, orow = 0, oc = 0;
};

bool key_less(const side_tile& x, const side_tile& y) {
    return std::tie(x.peer, x.tag, x.rows, x.cols) < std::tie(y.peer, y.tag, y.rows, y.cols);
}
bool key_equal(const side_tile& x, const side_tile& y) {
    return x.tag == y.tag && x.rows == y.rows && x.cols == y.cols;
}

// first cell of `split` overlapping index `a` (split[k] <= a < split[k+1])
int cell_of(const std::vector<int>& split, int a) {
    auto it = std::upper_bound(split.begin(), split.end(), a);
    return int(it - split.begin()) - 1;
}

// A layout seen in transform coordinates: transposed (rows <-> cols) when `t`.
struct view {
    const elayout* L;
    bool t;
    const std::vector<int>& rsplit() const { return t ? L->cols_split : L->rows_split; }
    const std::vector<int>& csplit() const { return t ? L->rows_split : L->cols_split; }
    int owner(int i, int j) const {
        int r = t ? j : i, c = t ? i : j;
        return L->owners[size_t(r) * size_t(L->nbc()) + size_t(c)];
    }
};

// The rule of a packed layout's tile (costa_hip.h, "MXFP4": the evenness rule, group 2; "MXFP6": the
// quad rule, group 4): the target-coordinate rectangle rr x cc of block b of L (seen transposed when
// `t`) starts at a whole number of packing groups from the block's pointer and has a whole number of
// them along L's stored-contiguous (packed) dimension.
void check_packed_tile(const elayout& L, const eblock& b, bool t, const interval& rr, const interval& cc) {
    const int g = packed_group(L.dtype);
    const bool packed_rows = L.ordering != 'R';             // 'C': rows share bytes
    const interval& own_r = t ? cc : rr;                    // back to L's own coordinates
    const interval& own_c = t ? rr : cc;
    const interval& iv = packed_rows ? own_r : own_c;
    const int at = iv.start - (packed_rows ? b.rows.start : b.cols.start);
    if (at % g == 0 && (iv.end - iv.start) % g == 0 && b.ld % g == 0) return;
    if (dtype_is_fp6(L.dtype))
        throw error(COSTA_ERR_ARG,
                    std::string("costa: FP6 quad: a tile splits a 3-byte group of the ") + dtype_name(L.dtype) +
                        " layout: its " + (packed_rows ? "rows [" : "columns [") + std::to_string(iv.start) + ", " +
                        std::to_string(iv.end) + ") start " + std::to_string(at) + " elements into the block at [" +
                        std::to_string(packed_rows ? b.rows.start : b.cols.start) + ", ...) (ld " +
                        std::to_string(b.ld) +
                        "); offsets, extents and ld along the packed dimension must be multiples of 4, which "
                        "makes the other layout's split points count through op");
    throw error(COSTA_ERR_ARG,
                std::string("costa: FP4 pair: a tile splits a byte of the FP4_E2M1 layout: its ") +
                    (packed_rows ? "rows [" : "columns [") + std::to_string(iv.start) + ", " +
                    std::to_string(iv.end) + ") start " + std::to_string(at) + " elements into the block at [" +
                    std::to_string(packed_rows ? b.rows.start : b.cols.start) +
                    ", ...) (ld " + std::to_string(b.ld) +
                    "); offsets, extents and ld along the packed dimension must be even, which makes the "
                    "other layout's split points count through op");
}

// decompose every local block of `src` (seen through `sv`) by the grid of `dst` (seen
// through `dv`) and append the tiles (utils.hpp:26-115)
// Under a mask each intersection tile is classified in target coordinates: wholly dropped tiles
// vanish, wholly kept ones are emitted as they are, and a tile the diagonal crosses is cut into row
// bands of kTriCut target rows from its first row; in each band the wholly dropped columns vanish,
// the wholly kept ones form one ordinary tile and the columns in between one edge tile (narrower
// than the band is tall).  The cut depends on the rectangle alone, so both sides of a pair make
// the same tiles with the same sort keys.
void decompose(const view& sv, const view& dv, int tag, const tri_mask& mk, std::vector<side_tile>& out) {
    out.reserve(out.size() + sv.L->blocks.size() * 4);
    const esize elem = elem_size(sv.L->dtype);  // of the layout being decomposed
    const bool packed = dtype_is_packed(sv.L->dtype);
    const auto& drs = dv.rsplit();
    const auto& dcs = dv.csplit();
    if (sv.rsplit().back() != drs.back() || sv.csplit().back() != dcs.back())
        throw error(COSTA_ERR_ARG, "costa::transform: layouts describe matrices of different sizes");
    const bool row_major = sv.L->ordering == 'R';
    for (const eblock& b : sv.L->blocks) {
        // block intervals in transform coordinates
        const interval vr = sv.t ? b.cols : b.rows;
        const interval vc = sv.t ? b.rows : b.cols;
        if (!vr.non_empty() || !vc.non_empty()) continue;
        const int i0 = cell_of(drs, vr.start), i1 = cell_of(drs, vr.end - 1) + 1;
        const int j0 = cell_of(dcs, vc.start), j1 = cell_of(dcs, vc.end - 1) + 1;
        for (int j = j0; j < j1; ++j) {
            const interval c(std::max(vc.start, dcs[j]), std::min(vc.end, dcs[j + 1]));
            if (c.empty()) continue;
            for (int i = i0; i < i1; ++i) {
                const interval r(std::max(vr.start, drs[i]), std::min(vr.end, drs[i + 1]));
                if (r.empty()) continue;
                const int peer = dv.owner(i, j);
                auto emit = [&](const interval& rr, const interval& cc, bool edge) {
                    if (packed) check_packed_tile(*sv.L, b, sv.t, rr, cc);  // no tile may split a packing group
                    // back to the stored orientation of the block (block.cpp:85-99)
                    const tile_side ts = sub_tile(reinterpret_cast<uint64_t>(b.data), b.ld, b.rows.start,
                                                  b.cols.start, row_major, sv.t, rr.start, rr.end,
                                                  cc.start, cc.end, elem);
                    out.push_back({peer, tag, rr, cc, reinterpret_cast<char*>(ts.ptr), b.ld, ts.n_rows,
                                   ts.n_cols, edge});
                };
                if (!mk.on) {
                    emit(r, c, false);
                    continue;
                }
                // v = j - i over the tile, i / j from the mask's origin (64-bit: k is any int)
                const int64_t k = mk.k;
                const int64_t i_lo = int64_t(r.start) - mk.orow, i_hi = int64_t(r.end) - 1 - mk.orow;
                const int64_t j_lo = int64_t(c.start) - mk.oc, j_hi = int64_t(c.end) - 1 - mk.oc;
                const int64_t v_min = j_lo - i_hi, v_max = j_hi - i_lo;
                if (mk.upper ? v_max < k : v_min > k) continue;  // wholly dropped
                if (mk.upper ? v_min >= k : v_max <= k) {        // wholly kept
                    emit(r, c, false);
                    continue;
                }
                auto clampc = [&](int64_t j) {  // relative column -> a column of [c.start, c.end]
                    return int(std::max<int64_t>(c.start, std::min<int64_t>(c.end, j + mk.oc)));
                };
                for (int b0 = r.start; b0 < r.end; b0 += kTriCut) {
                    const int b1 = std::min(r.end, b0 + kTriCut);
                    const interval rr(b0, b1);
                    const int64_t ib0 = int64_t(b0) - mk.orow, ib1 = int64_t(b1) - 1 - mk.orow;
                    if (mk.upper) {
                        // column j: wholly dropped when j - ib0 < k, wholly kept when j - ib1 >= k
                        const int e0 = clampc(k + ib0), e1 = std::max(e0, clampc(k + ib1));
                        if (e1 > e0) emit(rr, interval(e0, e1), true);
                        if (c.end > e1) emit(rr, interval(e1, c.end), false);
                    } else {
                        // column j: wholly kept when j - ib0 <= k, wholly dropped when j - ib1 > k
                        const int e0 = clampc(k + ib0 + 1), e1 = std::max(e0, clampc(k + ib1 + 1));
                        if (e0 > c.start) emit(rr, interval(c.start, e0), false);
                        if (e1 > e0) emit(rr, interval(e0, e1), true);
                    }
                }
            }
        }
    }
}

char upper(char c) { return char(std::toupper(static_cast<unsigned char>(c))); }

// costa_tile_op_t::order = 1 + rank of the tile in column-major order of its target
// coordinates (per tag): consecutive ranks walk down a column band, so each tile shares the
// partially used cache lines at its edges with the next one, on the source side (same source
// block) or on the destination side (same target block).
void set_order(std::vector<costa_tile_op_t>& ops, const std::vector<const side_tile*>& at) {
    // packed key (tag:16 | col start:24 | row start:24; matrix edges < 2^24) + index
    std::vector<std::pair<uint64_t, uint32_t>> k(ops.size());
    for (size_t i = 0; i < k.size(); ++i) {
        const side_tile& t = *at[i];
        k[i] = {(uint64_t(uint32_t(t.tag)) << 48) | (uint64_t(uint32_t(t.cols.start)) << 24) |
                    uint64_t(uint32_t(t.rows.start)),
                uint32_t(i)};
    }
    std::sort(k.begin(), k.end());
    for (size_t r = 0; r < k.size(); ++r) ops[k[r].second].order = uint32_t(r + 1);
}

}  // namespace

uint32_t scale_kind(costa_dtype_t dtype, const scal& s, bool copy_mode, bool conj) {
    switch (dtype) {
    case COSTA_FLOAT: return kind_t<float>(s, copy_mode, conj);
    case COSTA_DOUBLE: return kind_t<double>(s, copy_mode, conj);
    case COSTA_CFLOAT: return kind_t<std::complex<float>>(s, copy_mode, conj);
    case COSTA_CDOUBLE: return kind_t<std::complex<double>>(s, copy_mode, conj);
    case COSTA_INT32: return kind_t<int>(s, copy_mode, conj);
    // 2-byte types: the scalars are fp32 and the branches those of the FLOAT transform
    case COSTA_HALF: return kind_t<float>(s, copy_mode, conj);
    case COSTA_BFLOAT16: return kind_t<float>(s, copy_mode, conj);
    // 1-byte types: the same
    case COSTA_FP8_E4M3: return kind_t<float>(s, copy_mode, conj);
    case COSTA_FP8_E5M2: return kind_t<float>(s, copy_mode, conj);
    case COSTA_FP4_E2M1: return kind_t<float>(s, copy_mode, conj);
    case COSTA_FP6_E2M3: return kind_t<float>(s, copy_mode, conj);
    case COSTA_FP6_E3M2: return kind_t<float>(s, copy_mode, conj);
    }
    throw error(COSTA_ERR_ARG, "unknown dtype");
}

costa_tile_op_t make_tile_op(int n_rows, int n_cols, uint64_t src, int src_stride, bool src_cm,
                             uint64_t dst, int dst_stride, bool dst_cm, bool transpose, bool conj,
                             uint32_t kind, uint32_t slot, size_t elem) {
    return tile_op(n_rows, n_cols, src, src_stride, src_cm, dst, dst_stride, dst_cm, transpose, conj,
                   kind, slot, elem);
}

costa_tile_op_t make_tile_op(int n_rows, int n_cols, uint64_t src, int src_stride, bool src_cm,
                             uint64_t dst, int dst_stride, bool dst_cm, bool transpose, bool conj,
                             uint32_t kind, uint32_t slot, size_t src_elem, size_t dst_elem) {
    return tile_op(n_rows, n_cols, src, src_stride, src_cm, dst, dst_stride, dst_cm, transpose, conj,
                   kind, slot, src_elem, dst_elem);
}

std::vector<job_params> check_jobs(const std::vector<job>& jobs, int n_ranks, costa_dtype_t& dtype) {
    costa_dtype_t src;
    auto out = check_jobs(jobs, n_ranks, src, dtype);
    if (src != dtype)
        throw error(COSTA_ERR_ARG, "costa::transform: all layouts must share one element type");
    return out;
}

std::vector<job_params> check_jobs(const std::vector<job>& jobs, int n_ranks, costa_dtype_t& src_dtype,
                                   costa_dtype_t& dtype) {
    if (jobs.empty()) throw error(COSTA_ERR_ARG, "costa::transform: nothing scheduled");
    if (jobs.size() > 0xFFFF) throw error(COSTA_ERR_ARG, "costa::transform: too many layout pairs");
    src_dtype = jobs[0].A->dtype;
    dtype = jobs[0].C->dtype;
    if (any_packed(jobs)) {  // packed e2m1 / FP6: the MX transforms alone, one of the type's three pairs
        if (!(jobs.size() == 1 && jobs[0].mx))
            throw error(COSTA_ERR_ARG, std::string("costa::transform: ") +
                                           dtype_name(dtype_is_packed(src_dtype) ? src_dtype : dtype) +
                                           " layouts are taken by costa_hip_transform_mx alone, not " +
                                           dtype_name(src_dtype) + " (A) -> " + dtype_name(dtype) +
                                           " (C) here");
        if (!packed_pair(src_dtype, dtype))
            throw error(COSTA_ERR_ARG, std::string("costa_hip_transform_mx: no MX transform for ") +
                                           dtype_name(src_dtype) + " -> " + dtype_name(dtype));
    } else if (any_scaled(jobs)) {  // scaled transforms: their own set of pairs, one unmasked layout pair
        if (!scaled_pair(src_dtype, dtype))
            throw error(COSTA_ERR_ARG,
                        std::string("costa::transform_scaled: no scaled transform for ") +
                            dtype_name(src_dtype) + " (A) -> " + dtype_name(dtype) +
                            " (C): the pairs are FLOAT -> FLOAT, DOUBLE -> DOUBLE, and HALF, BFLOAT16, "
                            "FP8_E4M3 or FP8_E5M2 with itself or FLOAT");
        if (jobs.size() > 1)
            throw error(COSTA_ERR_ARG, "costa::transform_scaled: batches of scaled layout pairs are "
                                       "not supported");
        if (any_masked(jobs))
            throw error(COSTA_ERR_ARG, "costa::transform_scaled: a scaled transform takes no "
                                       "triangular mask");
    }
    // mixed precision: convert(A) in C's type; only the 2:1 pairs of one kind convert
    // (half precision: H -> H, FLOAT -> H, H -> FLOAT, computed in fp32; FP8: the same three shapes)
    const bool pair_ok =
        src_dtype == dtype || half_pair(src_dtype, dtype) || fp8_pair(src_dtype, dtype) ||
        packed_pair(src_dtype, dtype) ||
        (src_dtype == COSTA_FLOAT && dtype == COSTA_DOUBLE) || (src_dtype == COSTA_DOUBLE && dtype == COSTA_FLOAT) ||
        (src_dtype == COSTA_CFLOAT && dtype == COSTA_CDOUBLE) || (src_dtype == COSTA_CDOUBLE && dtype == COSTA_CFLOAT);
    if (!pair_ok)
        throw error(COSTA_ERR_ARG, std::string("costa::transform: cannot convert ") + dtype_name(src_dtype) +
                                       " (A) to " + dtype_name(dtype) +
                                       " (C): mixed transforms are FLOAT <-> DOUBLE, CFLOAT <-> CDOUBLE and "
                                       "FLOAT <-> HALF or BFLOAT16, and FLOAT <-> FP8_E4M3 or FP8_E5M2");
    const bool cplx = dtype_is_complex(dtype);
    std::vector<job_params> out;
    for (const job& jb : jobs) {
        if (jb.A->dtype != src_dtype || jb.C->dtype != dtype) {
            if (src_dtype == dtype && jb.A->dtype == jb.C->dtype)
                throw error(COSTA_ERR_ARG, "costa::transform: all layouts must share one element type");
            throw error(COSTA_ERR_ARG,
                        std::string("costa::transform: all layout pairs of a batch must share one (A, C) "
                                    "element-type pair: ") +
                            dtype_name(src_dtype) + " -> " + dtype_name(dtype) + " and " +
                            dtype_name(jb.A->dtype) + " -> " + dtype_name(jb.C->dtype));
        }
        for (const elayout* L : {jb.A, jb.C})
            for (int o : L->owners)
                if (o < 0 || o >= n_ranks)
                    throw error(COSTA_ERR_ARG,
                                "costa::transform: a block owner is outside the communicator");
        const char op = upper(jb.trans);
        if (op != 'N' && op != 'T' && op != 'C')
            throw error(COSTA_ERR_ARG, "costa::transform: trans must be 'N', 'T' or 'C'");
        const char ul = upper(jb.uplo);
        if (ul != 'A' && ul != 'U' && ul != 'L')
            throw error(COSTA_ERR_ARG, "costa::transform: uplo must be 'U' or 'L'");
        if (ul != 'A' && (dtype_is_half(src_dtype) || dtype_is_half(dtype)))
            throw error(COSTA_ERR_ARG,
                        std::string("costa::transform: triangular (masked) transforms take no 2-byte "
                                    "element type: ") +
                            dtype_name(src_dtype) + " (A), " + dtype_name(dtype) + " (C)");
        if (ul != 'A' && (dtype_is_fp8(src_dtype) || dtype_is_fp8(dtype)))
            throw error(COSTA_ERR_ARG,
                        std::string("costa::transform: triangular (masked) transforms take no 1-byte "
                                    "element type: ") +
                            dtype_name(src_dtype) + " (A), " + dtype_name(dtype) + " (C)");
        if (ul != 'A' && src_dtype != dtype)
            throw error(COSTA_ERR_ARG,
                        std::string("costa::transform: a triangular (masked) transform needs A and C of "
                                    "one element type, not ") +
                            dtype_name(src_dtype) + " and " + dtype_name(dtype));
        if (ul != 'A' && jobs.size() > 1)
            throw error(COSTA_ERR_ARG, "costa::transform: batches of triangular (masked) layout pairs "
                                       "are not supported");
        const bool tr = op != 'N';            // utils.cpp:9 (if_should_transpose)
        const bool cj = op == 'C' && cplx;    // communication_data.cpp:31-33
        out.push_back({tr, cj, jb.A->ordering == 'C', jb.C->ordering == 'C',
                       scale_kind(dtype, jb.s, true, cj), scale_kind(dtype, jb.s, false, cj)});
    }
    return out;
}

std::unique_ptr<plan> make_plan(const std::vector<job>& jobs, int rank, int n_ranks,
                                int loopback) {
    // loopback test mode: which of the rank's own tiles stay local
    auto stays_local = [&](const side_tile& m) {
        if (m.peer != rank) return false;
        if (loopback == 1) return false;
        if (loopback == 2) return ((m.rows.start / 7 + m.cols.start / 5) & 1) == 0;
        return true;
    };
    auto p = std::make_unique<plan>();
    p->rank = rank;
    p->n_ranks = n_ranks;
    using tag_info = job_params;
    const std::vector<tag_info> tags = check_jobs(jobs, n_ranks, p->src_dtype, p->dtype);
    // element sizes of A, of C and of the package (the narrower type crosses the exchange:
    // narrowing pairs convert in PACK, widening pairs in UNPACK); all equal for same-type plans.
    // FP8 pairs carry A's type, FLOAT -> Q too: its source is not rounded before the arithmetic,
    // which happens in UNPACK
    // (an FP4 side is half a byte per element, an FP6 side three quarters: esize; a packed package --
    // A holds FP4 or FP6 -- is counted in BYTES, `units`, so that no count, displacement or round
    // boundary falls inside a byte)
    const esize EA = elem_size(p->src_dtype), EC = elem_size(p->dtype);
    p->pkg_dtype = plan_pkg_dtype(p->src_dtype, p->dtype);
    const esize EP = elem_size(p->pkg_dtype);
    const bool packed_pkg = dtype_is_packed(p->pkg_dtype);
    auto units = [&](int64_t elems) { return pkg_units(p->pkg_dtype, elems); };
    std::vector<side_tile> send, recv;
    for (const job& jb : jobs) p->slots.push_back(jb.s);
    // prepare_to_send and prepare_to_recv are independent: the receive side runs on a second
    // thread when there are enough blocks to pay for it
    auto side = [&](bool send_side, std::vector<side_tile>& out) {
        for (size_t t = 0; t < jobs.size(); ++t) {
            const job& jb = jobs[t];
            const bool tr = tags[t].transpose;
            tri_mask mk;
            if (upper(jb.uplo) != 'A') {
                mk.on = true;
                mk.upper = upper(jb.uplo) == 'U';
                mk.k = jb.k;
                mk.orow = jb.C->rows_split.front();
                mk.oc = jb.C->cols_split.front();
            }
            if (send_side)
                decompose(view{jb.A, tr}, view{jb.C, false}, int(t), mk, out);  // prepare_to_send
            else
                decompose(view{jb.C, false}, view{jb.A, tr}, int(t), mk, out);  // prepare_to_recv
        }
        std::sort(out.begin(), out.end(), key_less);
    };
    size_t n_blocks = 0;
    for (const job& jb : jobs) n_blocks += jb.A->blocks.size() + jb.C->blocks.size();
    if (n_blocks >= 4096) {
        std::exception_ptr err;
        std::thread th([&] {
            try {
                side(false, recv);
            } catch (...) {
                err = std::current_exception();
            }
        });
        try {
            side(true, send);
        } catch (...) {
            th.join();
            throw;
        }
        th.join();
        if (err) std::rethrow_exception(err);
    } else {
        side(true, send);
        side(false, recv);
    }

    p->send_counts.assign(size_t(n_ranks), 0);
    p->recv_counts.assign(size_t(n_ranks), 0);
    p->send_displs.assign(size_t(n_ranks), 0);
    p->recv_displs.assign(size_t(n_ranks), 0);

    auto kind_of = [&](const tag_info& ti, bool n_rows_cols_transposes) {
        return n_rows_cols_transposes ? ti.kind_tr : ti.kind_copy;
    };
    auto will_tr = [](const tag_info& ti, bool src_cm, bool dst_cm) {
        return (ti.transpose && src_cm == dst_cm) || (!ti.transpose && src_cm != dst_cm);
    };

    // target coordinates of every op, for the locality hint (costa_tile_op_t::order)
    std::vector<const side_tile*> at_pack, at_unpack, at_local;
    // the edge op of a tile the mask's diagonal cuts, from its ordinary op (tile_op.hpp tri_op)
    auto edge_op = [&](const costa_tile_op_t& op, const side_tile& m, const tag_info& ti) {
        const job& jb = jobs[size_t(m.tag)];
        const int e = (m.cols.start - jb.C->cols_split.front()) - (m.rows.start - jb.C->rows_split.front());
        return tri_op(op, ti.a_cm, ti.transpose, upper(jb.uplo) == 'U', jb.k, e);
    };

    // ---- send side: local tiles stay, remote tiles are packed in sorted order ----
    std::vector<const side_tile*> local_src;
    int64_t off = 0;
    for (const side_tile& m : send) {
        if (stays_local(m)) {
            local_src.push_back(&m);
            continue;
        }
        const tag_info& ti = tags[size_t(m.tag)];
        const int64_t n = units(int64_t(m.n_rows) * m.n_cols);
        // copy_to_buffer: stored shape and ordering, dense, no transform (cpp:191-217)
        if (packed_pkg) {  // a copy of bytes: the extent and the pitch along the packed dimension in bytes
            auto pb = [&](int n) { return int(EP.bytes(uint64_t(n))); };  // (1/2 for FP4, 3/4 for FP6)
            p->pack_ops.push_back(tile_op(ti.a_cm ? pb(m.n_rows) : m.n_rows, ti.a_cm ? m.n_cols : pb(m.n_cols),
                                          uint64_t(m.ptr), pb(m.ld), ti.a_cm, uint64_t(off), 0, ti.a_cm, false,
                                          false, COSTA_SCALE_BITCOPY, 0, 1, 1));
        } else {
            p->pack_ops.push_back(tile_op(m.n_rows, m.n_cols, uint64_t(m.ptr), m.ld, ti.a_cm,
                                          EP.bytes(uint64_t(off)), 0, ti.a_cm, false, false,
                                          COSTA_SCALE_BITCOPY, 0, EA, EP));
        }
        at_pack.push_back(&m);
        p->send_counts[size_t(m.peer)] += n;
        off += n;
    }
    p->send_elems = off;

    // ---- receive side ----
    std::vector<const side_tile*> local_dst;
    off = 0;
    for (const side_tile& m : recv) {
        if (stays_local(m)) {
            local_dst.push_back(&m);
            continue;
        }
        const tag_info& ti = tags[size_t(m.tag)];
        const int64_t n = units(int64_t(m.n_rows) * m.n_cols);
        // copy_from_buffer(idx): the buffer holds the tile in A's stored shape/ordering
        // (cpp:219-244); dims swapped back when transposing
        const int nr = ti.transpose ? m.n_cols : m.n_rows;
        const int nc = ti.transpose ? m.n_rows : m.n_cols;
        const bool wt = will_tr(ti, ti.a_cm, ti.c_cm);
        const costa_tile_op_t op = tile_op(nr, nc, packed_pkg ? uint64_t(off) : EP.bytes(uint64_t(off)), 0, ti.a_cm,
                                           uint64_t(m.ptr), m.ld, ti.c_cm, ti.transpose, ti.conj, kind_of(ti, wt),
                                           uint32_t(m.tag), EP, EC);
        if (m.edge) {
            p->unpack_tri.push_back(edge_op(op, m, ti));
        } else {
            p->unpack_ops.push_back(op);
            at_unpack.push_back(&m);
        }
        p->recv_counts[size_t(m.peer)] += n;
        off += n;
    }
    p->recv_elems = off;

    // ---- local pairs (copy_local_blocks, cpp:251-302): same key order on both sides ----
    if (local_src.size() != local_dst.size())
        throw error(COSTA_ERR_INTERNAL, "costa: local tile lists of the two sides differ");
    for (size_t k = 0; k < local_src.size(); ++k) {
        const side_tile& s = *local_src[k];
        const side_tile& d = *local_dst[k];
        if (!key_equal(s, d) || s.edge != d.edge ||
            int64_t(s.n_rows) * s.n_cols != int64_t(d.n_rows) * d.n_cols)
            throw error(COSTA_ERR_INTERNAL, "costa: local tiles do not pair up");
        const tag_info& ti = tags[size_t(s.tag)];
        const bool wt = will_tr(ti, ti.a_cm, ti.c_cm);
        const costa_tile_op_t op = tile_op(s.n_rows, s.n_cols, uint64_t(s.ptr), s.ld, ti.a_cm,
                                           uint64_t(d.ptr), d.ld, ti.c_cm, ti.transpose, ti.conj,
                                           kind_of(ti, wt), uint32_t(s.tag), EA, EC);
        if (d.edge) {
            p->local_tri.push_back(edge_op(op, d, ti));
            p->local_elems += tri_kept(p->local_tri.back());
            continue;
        }
        p->local_ops.push_back(op);
        at_local.push_back(&d);
        p->local_elems += int64_t(s.n_rows) * s.n_cols;
    }

    for (int r = 1; r < n_ranks; ++r) {
        p->send_displs[size_t(r)] = p->send_displs[size_t(r - 1)] + p->send_counts[size_t(r - 1)];
        p->recv_displs[size_t(r)] = p->recv_displs[size_t(r - 1)] + p->recv_counts[size_t(r - 1)];
    }
    set_order(p->pack_ops, at_pack);
    set_order(p->unpack_ops, at_unpack);
    set_order(p->local_ops, at_local);
    // algorithmic bytes: each side of an op at its own element size
    for (auto& op : p->local_ops) p->local_bytes += op_alg_bytes(op, EA, EC);
    for (auto& op : p->pack_ops)  // (a packed package's pack ops are byte ops)
        p->pack_bytes += packed_pkg ? op_alg_bytes(op, 1, 1) : op_alg_bytes(op, EA, EP);
    for (auto& op : p->unpack_ops) p->unpack_bytes += op_alg_bytes(op, EP, EC);
    for (auto& t : p->local_tri) p->local_bytes += op_alg_bytes(t, EC);  // kept elements only
    for (auto& t : p->unpack_tri) p->unpack_bytes += op_alg_bytes(t, EC);
    if (any_scaled(jobs)) {
        // a scaled plan is the ordinary plan with every LOCAL and UNPACK op moved, in order and
        // with its locality hint, to the scaled lists next to its target coordinates
        // (tile_op.hpp scaled_op); the pack list and the exchange geometry stay as they are
        p->scaled = true;
        auto move = [&](std::vector<costa_tile_op_t>& ops, const std::vector<const side_tile*>& at,
                        std::vector<costa_scaled_op_t>& out) {
            out.reserve(ops.size());
            for (size_t i = 0; i < ops.size(); ++i) {
                const side_tile& m = *at[i];
                const job& jb = jobs[size_t(m.tag)];
                const tag_info& ti = tags[size_t(m.tag)];
                out.push_back(scaled_op(ops[i], ti.a_cm, ti.transpose,
                                        m.rows.start - jb.C->rows_split.front(),
                                        m.cols.start - jb.C->cols_split.front()));
            }
            ops.clear();
        };
        move(p->local_ops, at_local, p->local_scaled);
        move(p->unpack_ops, at_unpack, p->unpack_scaled);
    }
    return p;
}

}  // namespace engine
}  // namespace costa
