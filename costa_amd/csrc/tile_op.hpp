// One tile of a transform as a costa_tile_op_t: the sub-tile address inside its block and the
// normalisation of copy_and_transform's dispatch.  Shared by the host planner (plan.cpp) and
// the device planner (device_plan.hip), so both emit bit-identical ops.
#pragma once

#include <cstdint>

#include "costa_hip.h"

#if defined(__HIPCC__)
#define COSTA_HD __host__ __device__
#else
#define COSTA_HD
#endif

namespace costa {
namespace engine {

// The size of one element of a side, in quarter-bytes: COSTA_FP4_E2M1 packs two elements into a byte
// (costa_hip.h, "MXFP4") and the FP6 types four into three bytes ("MXFP6"), so no byte count says it.
// A plain byte count converts implicitly; bytes(n) is exact for a packed side because its rule (the
// evenness rule, the quad rule) keeps every n it is asked about a multiple of the packing group.
struct esize {
    uint64_t qb;  // quarter-bytes per element
    COSTA_HD constexpr esize(uint64_t bytes) : qb(4 * bytes) {}
    // `bits` per element of a packed sub-byte type: 4 or 6
    COSTA_HD static constexpr esize packed(unsigned bits) {
        esize e(0);
        e.qb = bits / 2;
        return e;
    }
    COSTA_HD constexpr uint64_t bytes(uint64_t n) const { return n * qb / 4; }
};

// The stored-orientation sub-tile of a block for the target-coordinate rectangle
// [r0, r1) x [c0, c1) of a view that is transposed when `t` (block.cpp:72-111).
struct tile_side {
    uint64_t ptr;         // first element
    int ld;
    int n_rows, n_cols;   // stored orientation
};

COSTA_HD inline tile_side sub_tile(uint64_t data, int ld, int block_row0, int block_col0,
                                   bool row_major, bool t, int r0, int r1, int c0, int c1,
                                   esize elem) {
    // back to the stored orientation of the block
    const int sr0 = t ? c0 : r0, sr1 = t ? c1 : r1;
    const int sc0 = t ? r0 : c0, sc1 = t ? r1 : c1;
    const int64_t dr = sr0 - block_row0, dc = sc0 - block_col0;
    const int64_t off = row_major ? dr * ld + dc : dc * ld + dr;
    return {data + uint64_t(off * int64_t(elem.qb) / 4), ld, sr1 - sr0, sc1 - sc0};
}

// copy_and_transform (memory_utils.hpp:339-412) as one op: an ordering mismatch is itself a
// transpose and cancels an explicit one (:353-367); stride 0 means the default stride
// (:330-337, 370-381); a transposing op never takes the memcpy branch.
// Converting ops (mixed-precision transforms) have a source element of `src_elem` bytes and a
// destination element of `dst_elem`: each side's VEC flag follows its own byte alignment.
COSTA_HD inline costa_tile_op_t tile_op(int n_rows, int n_cols, uint64_t src, int src_stride,
                                        bool src_cm, uint64_t dst, int dst_stride, bool dst_cm,
                                        bool transpose, bool conj, uint32_t kind, uint32_t slot,
                                        esize src_elem, esize dst_elem) {
    const bool will_transpose = (transpose && src_cm == dst_cm) || (!transpose && src_cm != dst_cm);
    if (dst_stride == 0) {
        const int r = will_transpose ? n_cols : n_rows, c = will_transpose ? n_rows : n_cols;
        dst_stride = dst_cm ? r : c;
    }
    if (src_stride == 0) src_stride = src_cm ? n_rows : n_cols;
    costa_tile_op_t op{};
    op.src = src;
    op.dst = dst;
    op.nf = src_cm ? n_rows : n_cols;  // contiguous extent of the source
    op.ns = src_cm ? n_cols : n_rows;
    op.lds = src_stride;
    op.ldd = dst_stride;
    if (will_transpose && kind == COSTA_SCALE_BITCOPY) kind = COSTA_SCALE_ALPHA;  // never memcpy
    op.flags = (will_transpose ? COSTA_TILE_TRANSPOSE : 0u) | (conj ? COSTA_TILE_CONJ : 0u) |
               (kind << COSTA_SCALE_SHIFT) | (slot << COSTA_SLOT_SHIFT);
    if (src % 16 == 0 && src_elem.bytes(uint64_t(src_stride)) % 16 == 0) op.flags |= COSTA_TILE_VEC_SRC;
    if (dst % 16 == 0 && dst_elem.bytes(uint64_t(dst_stride)) % 16 == 0) op.flags |= COSTA_TILE_VEC_DST;
    return op;
}

COSTA_HD inline costa_tile_op_t tile_op(int n_rows, int n_cols, uint64_t src, int src_stride,
                                        bool src_cm, uint64_t dst, int dst_stride, bool dst_cm,
                                        bool transpose, bool conj, uint32_t kind, uint32_t slot,
                                        esize elem) {
    return tile_op(n_rows, n_cols, src, src_stride, src_cm, dst, dst_stride, dst_cm, transpose, conj,
                   kind, slot, elem, elem);
}

// The edge tile of a triangular transform.  `op` is the tile's ordinary op; its first element sits
// at target (C) position (r0, c0) counted from the mask's origin, `e` = c0 - r0, and the mask keeps
// target element (i, j) when j - i >= k ('U') or j - i <= k ('L').  The op's source is A's stored
// tile (or its dense image in the package), column-major when `src_cm`, seen transposed when
// `transpose` (the job's op != 'N'): its fast index f walks target rows when src_cm != transpose,
// target columns otherwise.  So j - i = e + (s - f) or e - (s - f), and the mask becomes
// s - f >= diag or s - f <= diag (COSTA_TRI_LE) for every ordering / transpose combination.
COSTA_HD inline costa_tri_op_t tri_op(const costa_tile_op_t& op, bool src_cm, bool transpose, bool upper,
                                      int k, int e) {
    costa_tri_op_t t{};
    t.op = op;
    const bool f_is_row = src_cm != transpose;
    // f_is_row:  'U' s - f >= k - e,  'L' s - f <= k - e;  else:  'U' s - f <= e - k,  'L' s - f >= e - k
    const int64_t d = f_is_row ? int64_t(k) - e : int64_t(e) - k;
    const int64_t lim = int64_t(1) << 30;  // (beyond the op either way: clamped, no overflow)
    t.diag = int32_t(d < -lim ? -lim : d > lim ? lim : d);
    if (f_is_row != upper) t.op.flags |= COSTA_TRI_LE;
    return t;
}

// The op of a scaled transform.  `op` is the tile's ordinary op; its source element (0, 0) sits at
// target (C) position (r0, c0) counted from the first row and column of C's matrix.  As in tri_op(),
// the source's fast index f walks target rows when src_cm != transpose (COSTA_SCALED_F_ROWS).
COSTA_HD inline costa_scaled_op_t scaled_op(const costa_tile_op_t& op, bool src_cm, bool transpose, int r0,
                                            int c0) {
    costa_scaled_op_t t{};
    t.op = op;
    t.row0 = r0;
    t.col0 = c0;
    if (src_cm != transpose) t.op.flags |= COSTA_SCALED_F_ROWS;
    return t;
}

// the ordinary op inside each op type
COSTA_HD inline const costa_tile_op_t& tile_of(const costa_tile_op_t& o) { return o; }
COSTA_HD inline const costa_tile_op_t& tile_of(const costa_tri_op_t& o) { return o.op; }
COSTA_HD inline const costa_tile_op_t& tile_of(const costa_scaled_op_t& o) { return o.op; }
COSTA_HD inline costa_tile_op_t& tile_of(costa_tile_op_t& o) { return o; }
COSTA_HD inline costa_tile_op_t& tile_of(costa_tri_op_t& o) { return o.op; }
COSTA_HD inline costa_tile_op_t& tile_of(costa_scaled_op_t& o) { return o.op; }
COSTA_HD inline const costa_tile_op_t& tile_of(const costa_dual_op_t& o) { return o.s.op; }
COSTA_HD inline costa_tile_op_t& tile_of(costa_dual_op_t& o) { return o.s.op; }

// kept elements of an edge op
COSTA_HD inline int64_t tri_kept(const costa_tri_op_t& t) {
    const bool le = t.op.flags & COSTA_TRI_LE;
    int64_t n = 0;
    for (int64_t s = 0; s < t.op.ns; ++s) {
        // GE: f <= s - diag;  LE: f >= s - diag
        const int64_t x = s - t.diag;
        const int64_t c = le ? int64_t(t.op.nf) - x : x + 1;
        n += c < 0 ? 0 : c > t.op.nf ? t.op.nf : c;
    }
    return n;
}

// algorithmic HBM bytes of one op: read + write (+ read of the target when beta != 0)
COSTA_HD inline int64_t op_alg_bytes(const costa_tile_op_t& op, esize elem) {
    const uint32_t k = (op.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const int64_t n = int64_t(op.nf) * op.ns;
    return int64_t(elem.bytes(uint64_t(n))) * (1 + (k != COSTA_SCALE_ZERO) + (k == COSTA_SCALE_AXPBY));
}
// ... of a converting op: each side at its own element size
COSTA_HD inline int64_t op_alg_bytes(const costa_tile_op_t& op, esize src_elem, esize dst_elem) {
    const uint32_t k = (op.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const int64_t n = int64_t(op.nf) * op.ns;
    return int64_t(src_elem.bytes(uint64_t(n))) * (k != COSTA_SCALE_ZERO) +
           int64_t(dst_elem.bytes(uint64_t(n))) * (1 + (k == COSTA_SCALE_AXPBY));
}

// ... of an edge op: kept elements only
COSTA_HD inline int64_t op_alg_bytes(const costa_tri_op_t& t, esize elem) {
    const uint32_t k = (t.op.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    return int64_t(elem.bytes(uint64_t(tri_kept(t)))) * (1 + (k != COSTA_SCALE_ZERO) + (k == COSTA_SCALE_AXPBY));
}

}  // namespace engine
}  // namespace costa
