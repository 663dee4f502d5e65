// Work lists of the strip kernel families (convert_kernels.hip, half_kernels.hip, fp8_kernels.hip,
// tri_kernels.hip, scaled_kernels.hip, mx_kernels.hip, mx_dual_kernels.hip; launched by strip_launch.hpp): the
// alignment rule of the VEC flags and the one builder behind build_convert_work, build_tri_work,
// build_scaled_work and build_dual_work.
// Integer arithmetic on op descriptors only: no HIP in it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "engine.hpp"
#include "tile_op.hpp"

namespace costa {
namespace engine {

// A side of an op may use vector accesses (its VEC flag) when its first element and its leading
// dimension are aligned to the side's strip: V elements of that side's size, 16 bytes at most.
//   family                      V                     source side          destination side
//   2:1 real or complex pair    16 / wider element    16 wider, 8 narrower the same rule
//   half pair                   4                     8 on a 2-byte side, 16 on fp32
//   FP8 with FLOAT              4                     4 on the 1-byte side, 16 on fp32
//   Q -> Q                      16 (its whole copies) 16                   16
//   scaled pair                 4                     min(16, 4 x element size)
//   MX pair with packed FP4     4                     2 on the FP4 side (a strip is 2 bytes)
//   MX pair with packed FP6     4                     1 on the FP6 side: a strip is 3 bytes at any
//                                                     address, moved by a 2-byte and a 1-byte access
//                                                     that ask nothing of it, so the flag is
//                                                     always set there (vacuous) and a whole sub-tile
//                                                     takes the FULL path on the other side's flag alone
//   tri                         16 / element          16                   16
enum class strip_family { pair, scaled, tri };
struct strip_align {
    uint64_t src, dst;
};
inline strip_align strip_alignment(strip_family fam, uint64_t es, uint64_t ed) {
    uint64_t v = 4;
    if (fam == strip_family::tri) v = 16 / es;
    else if (fam == strip_family::pair && es != ed) v = 16 / std::max(es, ed);
    else if (fam == strip_family::pair && es == 1) v = 16;
    return {std::min<uint64_t>(16, v * es), std::min<uint64_t>(16, v * ed)};
}

// what the builder does with one sub-tile: leave it out, list it, or list it as `whole` (tri: every
// element kept)
enum class strip_sub { skip, listed, whole };
struct all_listed {
    template <typename Op>
    strip_sub operator()(const Op&, int64_t, int64_t) const {
        return strip_sub::listed;
    }
};

// The work list of `ops` on bf x bs sub-tiles.  `ordered` = the non-empty ops with a listed sub-tile,
// each side's VEC flag set from its actual address (base + offset), leading dimension and `align`;
// `work` = (index in ordered << 32) | sub-tile, sub-tiles in ascending order per op -- with
// WHOLE_BIT (index << 32) | sub-tile << 1 | whole.  `sub_of(op, i, j)` classifies sub-tile
// (i along f, j along s).  dst_order: the items sorted by the address of their sub-tile's first
// destination element (stable), as the ordinary LOCAL list of a triangular plan (engine.cpp
// build_work dst_order).  `what` names the list in the error text.
template <bool WHOLE_BIT = false, typename Op, typename SubOf = all_listed>
strip_list build_strip_work(const char* what, const std::vector<Op>& ops, uint64_t src_base, uint64_t dst_base,
                            int bf_, int bs_, esize es, esize ed, strip_align align,
                            std::vector<Op>& ordered, std::vector<uint64_t>& work, SubOf sub_of = SubOf(),
                            bool dst_order = false) {
    const int64_t bf = bf_, bs = bs_;
    constexpr int SHIFT = WHOLE_BIT ? 1 : 0;
    strip_list l;
    ordered.clear();
    work.clear();
    ordered.reserve(ops.size());
    for (const Op& in : ops) {
        if (tile_of(in).nf <= 0 || tile_of(in).ns <= 0) continue;
        if (tile_of(in).lds < 0 || tile_of(in).ldd < 0)
            throw error(COSTA_ERR_ARG, "costa: negative leading dimension");
        Op t = in;
        costa_tile_op_t& op = tile_of(t);
        op.flags &= ~uint32_t(COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST);
        if ((src_base + op.src) % align.src == 0 && es.bytes(uint64_t(op.lds)) % align.src == 0)
            op.flags |= COSTA_TILE_VEC_SRC;
        if ((dst_base + op.dst) % align.dst == 0 && ed.bytes(uint64_t(op.ldd)) % align.dst == 0)
            op.flags |= COSTA_TILE_VEC_DST;
        const uint64_t idx = ordered.size();
        const int64_t nbf = (int64_t(op.nf) + bf - 1) / bf, nbs = (int64_t(op.ns) + bs - 1) / bs;
        if (idx >> 32 || (nbf * nbs) >> (32 - SHIFT))
            throw error(COSTA_ERR_ARG, std::string("costa: ") + what + " list too long for its work items");
        bool used = false;
        for (int64_t q = 0; q < nbf * nbs; ++q) {
            const strip_sub k = sub_of(t, q % nbf, q / nbf);
            if (k == strip_sub::skip) continue;
            if (!used) {
                ordered.push_back(t);
                used = true;
                if (op.flags & COSTA_TILE_TRANSPOSE) l.any_transpose = true;
            }
            work.push_back(idx << 32 | uint64_t(q) << SHIFT | uint64_t(WHOLE_BIT && k == strip_sub::whole));
        }
    }
    if (dst_order && work.size() > 1) {
        std::vector<std::pair<uint64_t, uint64_t>> key(work.size());
        for (size_t x = 0; x < key.size(); ++x) {
            const costa_tile_op_t& op = tile_of(ordered[size_t(work[x] >> 32)]);
            const uint64_t q = (work[x] & 0xFFFFFFFFull) >> SHIFT, nbf = uint64_t((op.nf + bf - 1) / bf);
            const int64_t f0 = int64_t(q % nbf) * bf, s0 = int64_t(q / nbf) * bs;
            const int64_t at = op.flags & COSTA_TILE_TRANSPOSE ? f0 * op.ldd + s0 : s0 * op.ldd + f0;
            key[x] = {op.dst + ed.bytes(uint64_t(at)), work[x]};
        }
        std::stable_sort(key.begin(), key.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (size_t x = 0; x < key.size(); ++x) work[x] = key[x].second;
    }
    l.n_items = int64_t(work.size());
    return l;
}

}  // namespace engine
}  // namespace costa
