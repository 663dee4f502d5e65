// Invariants of the work lists (engine.cpp build_work), without a GPU (block addresses are never
// touched).  Run by tests/test_work_lists.py.
//   cfg 5 'N' (copy list) and 'T' (transposing list) on BASELINE cfg 5's geometry:
//     * the ops that take a sub-tiled shape are the ones the classification rules name (the
//       'T' list's aligned ops of at least half a medium sub-tile);
//     * every piece fits the wavefront budget the library uses (tiny_copy_budget,
//       tiny_lds_budget; staged pitch nf | 1);
//     * the pieces of every op (found by its unique locality hint) lie inside it and add up to it;
//     * order: by the op's destination address within at most 8 column bands (copy and
//       transposing lists alike), pack lists by the op's source address;
//     * two builds give byte-identical lists (the threaded cut is deterministic).
//   a sub-list of every 8th cfg 5 op (what one exchange round's pack / unpack list looks like:
//     hints sparse in the list, so the comparison sort replaces the counting sort): the same.
//   unaligned large ops (fp32, lld % 4 != 0): transposes into unaligned destinations take the
//     skew shape; other ops up to kUnalignedWaveCap large sub-tiles are cut into wavefront
//     pieces (the same checks), bigger ones stay on the large shape.
//   run with COSTA_MERGE=0 (ops that continue each other stay apart: every op has one parent);
//   `work_check merge` checks the merging itself; `work_check cover` that the sub-tiled work items
//   of the default lists (panels, skew XCD groups, merged ragged blocks) cover their ops exactly;
//   `work_check rounds` the exchange round of every pack and unpack op of multi-rank plans;
//   `work_check extents` lists whose leading dimensions pass 2^32 bytes / 2^31 elements.
// Prints "ok" and exits 0, or prints the first violation and exits 1.
#include <chrono>
#include <complex>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <random>
#include <string>
#include <vector>

#include "engine.hpp"
#include "tile_op.hpp"

using namespace costa;
using namespace costa::engine;

static std::vector<int> splits(uint64_t seed, int lo, int hi, int n) {
    std::mt19937_64 r(seed);
    std::uniform_int_distribution<int> d(lo, hi);
    std::vector<int> s{0};
    while (s.back() < n) s.push_back(std::min(n, s.back() + d(r)));
    return s;
}

template <typename T = float>
static grid_layout<T> layout(const std::vector<int>& rs, const std::vector<int>& cs, uint64_t base,
                             uint64_t gap = 0) {
    const int nr = int(rs.size()) - 1, nc = int(cs.size()) - 1;
    std::vector<int> own(size_t(nr) * size_t(nc), 0);
    std::vector<block_t> blocks;
    uint64_t off = 0;
    for (int i = 0; i < nr; ++i)
        for (int j = 0; j < nc; ++j) {
            const int rows = rs[size_t(i) + 1] - rs[size_t(i)], cols = cs[size_t(j) + 1] - cs[size_t(j)];
            blocks.push_back({reinterpret_cast<void*>(base + sizeof(T) * off), rows, i, j});
            off += (uint64_t(rows) * uint64_t(cols) + 63) / 64 * 64 + gap;
        }
    return custom_layout<T>(nr, nc, rs.data(), cs.data(), own.data(), int(blocks.size()),
                                blocks.data(), 'C');
}

#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            std::printf("FAIL %s: ", name.c_str());    \
            std::printf(__VA_ARGS__);                  \
            std::printf("\n");                         \
            return false;                              \
        }                                              \
    } while (0)

// hints of the ops the classification rules put on a sub-tiled shape: aligned ops of at least
// half a large sub-tile, unaligned ones above kUnalignedWaveCap sub-tiles, transposes into
// unaligned destinations (the skew shape, engine.cpp build_work), and in lists that transpose,
// aligned transposing ops of at least half a medium sub-tile
static std::set<uint32_t> expected_shaped(costa_dtype_t dt, const std::vector<costa_tile_op_t>& ops,
                                          bool pack = false) {
    bool tr = false;
    for (const auto& o : ops) tr = tr || (o.flags & COSTA_TILE_TRANSPOSE);
    shape_dims sh;
    tile_shapes(dt, tr, &sh);
    const int64_t E = int64_t(dtype_size(dt)), big = int64_t(sh.cf) * sh.cs, med = int64_t(sh.bf_m) * sh.bs_m;
    const uint32_t both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    const int64_t skew_elems = int64_t(sh.bf_k) * sh.bs_k;
    std::set<uint32_t> large, medium;
    for (const auto& o0 : ops) {
        costa_tile_op_t o = o0;
        const int64_t e = int64_t(o.nf) * o.ns;
        // 4-byte sources off the grid read as 16-byte vectors (engine.cpp build_work), ops of at
        // least one large sub-tile
        if (E == 4 && e >= big && o.src % 4 == 0) o.flags |= COSTA_TILE_VEC_SRC;
        const bool al = (o.flags & both) == both, t = o.flags & COSTA_TILE_TRANSPOSE;
        const uint32_t kind = (o.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
        const bool off_granule = o.dst % 64 != 0 || (uint64_t(o.ldd) * uint64_t(E)) % 64 != 0;
        if (skew_elems > 0 && e > 0 && t && (!(o.flags & COSTA_TILE_VEC_DST) || off_granule) &&
            o.dst % uint64_t(E) == 0 && 2 * e >= skew_elems) {
            large.insert(o.order);
            continue;
        }
        const bool tiny = (t ? int64_t(o.nf | 1) * o.ns * E <= tiny_lds_budget() : e * E <= tiny_copy_budget(E, !pack));
        const bool lg = 2 * e >= big && (al || e > kUnalignedWaveCap * big) && !tiny;
        if (lg) large.insert(o.order);
        else if (med > 0 && al && t && 2 * e >= med) medium.insert(o.order);
    }
    if (medium.size() >= 4096) large.insert(medium.begin(), medium.end());  // engine.cpp kMinMediumOps
    return large;
}

static int64_t big_elems(costa_dtype_t dt, const std::vector<costa_tile_op_t>& ops) {
    bool tr = false;
    for (const auto& o : ops) tr = tr || (o.flags & COSTA_TILE_TRANSPOSE);
    shape_dims sh;
    tile_shapes(dt, tr, &sh);
    return int64_t(sh.cf) * sh.cs;  // the large class (engine.cpp build_work)
}

// `ops` must carry unique, non-zero hints; expect_large: ops that must go to a sub-tiled shape
static bool check_list(const std::string& name, costa_dtype_t dt, const std::vector<costa_tile_op_t>& ops,
                       const std::set<uint32_t>& shaped, bool pack = false) {
    const int64_t E = int64_t(dtype_size(dt));
    std::vector<costa_tile_op_t> ord, ord2;
    std::vector<uint64_t> work, work2;
    const list_kind kind = pack ? list_pack : list_local;
    const work_split w = build_work(dt, ops, ord, work, kind);
    build_work(dt, ops, ord2, work2, kind);
    // (skew ops that continue each other are merged: fewer shaped ops than parents)
    CHECK(w.tiny_first <= int64_t(shaped.size()) && (w.tiny_first == 0) == shaped.empty(),
          "%lld ops on the sub-tiled shapes, expected %zu", (long long)w.tiny_first, shaped.size());
    CHECK(ord.size() == ord2.size() && work == work2 &&
              std::memcmp(ord.data(), ord2.data(), ord.size() * sizeof(costa_tile_op_t)) == 0,
          "two builds differ");
    std::map<uint32_t, const costa_tile_op_t*> parent;
    for (const auto& o : ops) CHECK(o.order > 0 && parent.emplace(o.order, &o).second, "hint %u not unique", o.order);
    std::map<uint32_t, int64_t> area;
    int restarts = 0;  // the large ops, then the medium ones: each run whole, in hint order
    int64_t shaped_area = 0, want_area = 0;
    for (const auto& o : ops)
        if (shaped.count(o.order)) want_area += int64_t(o.nf) * o.ns;
    for (int64_t i = 0; i < w.tiny_first; ++i) {
        const costa_tile_op_t& s = ord[size_t(i)];
        CHECK(parent.count(s.order) && shaped.count(s.order), "shaped op %lld has no shaped parent", (long long)i);
        costa_tile_op_t q = *parent[s.order];
        if (E == 4 && int64_t(q.nf) * q.ns >= big_elems(dt, ops) && q.src % 4 == 0) q.flags |= COSTA_TILE_VEC_SRC;
        // an op merged from tiles that continue each other (merge_filled / merge_adjacent, copy or
        // transpose mode) starts at the tile whose hint it keeps
        const bool merged = s.src == q.src && s.dst == q.dst && s.flags == q.flags && s.lds == q.lds &&
                            s.ldd == q.ldd && s.nf >= q.nf && s.ns >= q.ns;
        CHECK(std::memcmp(&s, &q, sizeof(s)) == 0 || merged, "shaped op %lld", (long long)i);
        restarts += i > 0 && ord[size_t(i) - 1].order > s.order;
        CHECK(restarts <= 2, "shaped op %lld out of hint order", (long long)i);
        shaped_area += int64_t(s.nf) * s.ns;
    }
    CHECK(shaped_area == want_area, "shaped ops cover %lld of %lld elements", (long long)shaped_area,
          (long long)want_area);
    uint64_t last_key = 0;
    int band_restarts = 0;
    for (int64_t i = w.tiny_first; i < w.tiny_first + w.n_tiny; ++i) {
        const costa_tile_op_t& s = ord[size_t(i)];
        const bool tr = s.flags & COSTA_TILE_TRANSPOSE;
        const int64_t bytes = tr ? int64_t(s.nf | 1) * s.ns * E : int64_t(s.nf) * s.ns * E;
        CHECK(bytes <= (tr ? tiny_lds_budget() : tiny_copy_budget(E, !pack)), "piece %lld over budget (%lld B)",
              (long long)i, (long long)bytes);
        auto it = parent.find(s.order);
        CHECK(it != parent.end(), "piece %lld has no parent", (long long)i);
        const costa_tile_op_t& q = *it->second;
        CHECK(s.lds == q.lds && s.ldd == q.ldd && s.src >= q.src, "piece %lld strides", (long long)i);
        const int64_t off = int64_t(s.src - q.src) / E, s0 = off / q.lds, f0 = off % q.lds;
        CHECK(f0 + s.nf <= q.nf && s0 + s.ns <= q.ns, "piece %lld outside its op", (long long)i);
        const uint64_t dst = q.dst + uint64_t((tr ? f0 * q.ldd + s0 : s0 * q.ldd + f0) * E);
        CHECK(s.dst == dst, "piece %lld destination", (long long)i);
        area[s.order] += int64_t(s.nf) * s.ns;
        // wave_knobs::sort 5; other lists in 8 XCD column bands (wave_knobs::xcd_bands), each
        // in destination order
        const uint64_t key = pack ? q.src : q.dst;
        if (key < last_key) ++band_restarts;
        CHECK(band_restarts <= (pack ? 0 : 7), "piece %lld out of order", (long long)i);
        last_key = key;
    }
    for (const auto& o : ops)
        CHECK(shaped.count(o.order) || area[o.order] == int64_t(o.nf) * o.ns, "op %u: pieces cover %lld of %lld",
              o.order, (long long)area[o.order], (long long)(int64_t(o.nf) * o.ns));
    std::printf("%s: %zu ops -> %lld large, %lld pieces\n", name.c_str(), ops.size(),
                (long long)w.tiny_first, (long long)w.n_tiny);
    return true;
}

static std::unique_ptr<plan> plan_of(const elayout& a, const elayout& c, char op, float alpha, float beta) {
    job j;
    j.A = &a;
    j.C = &c;
    j.trans = op;
    std::memcpy(j.s.alpha.data(), &alpha, 4);
    std::memcpy(j.s.beta.data(), &beta, 4);
    return make_plan({j}, 0, 1);
}

// merging (engine.cpp merge_adjacent, run with COSTA_MERGE unset): a 4096^2 matrix on one rank
// with 24^2 blocks, 'T' and 'N', fp32 and fp64: every tile continues its neighbours in source and
// destination, so the list becomes one op on the large shape; with a ragged last block row
// (4100^2: blocks of 24 and 20 rows) the ops still cover every element once
static bool check_merge() {
    const std::string name = "merge";
    for (int m : {4096, 4100})
        for (char op : {'T', 'N'}) {
            auto A = block_cyclic_layout<float>(m, m, 24, 24, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                                reinterpret_cast<float*>(uint64_t(1) << 40), m, 'C', 0);
            auto C = block_cyclic_layout<float>(m, m, 24, 24, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                                reinterpret_cast<float*>(uint64_t(1) << 41), m, 'C', 0);
            elayout ea = erase(A), ec = erase(C);
            auto p = plan_of(ea, ec, op, 1.f, 0.f);
            std::vector<costa_tile_op_t> ord;
            std::vector<uint64_t> work;
            const work_split w = build_work(p->dtype, p->local_ops, ord, work, list_local);
            int64_t area = 0;
            for (const auto& o : ord) area += int64_t(o.nf) * o.ns;
            // (pieces of wavefront ops are in `ord` after tiny_first; shaped ops before)
            CHECK(area == int64_t(m) * m, "%c %d: ops cover %lld of %lld elements", op, m, (long long)area,
                  (long long)int64_t(m) * m);
            // ('N' with columns off the 64-byte grid: the merged op is then cut at the granules,
            // engine.cpp granule_split -- 4 column classes, their heads as wavefront pieces)
            const bool gran = op == 'N' && (int64_t(m) * 4) % 64 != 0;
            CHECK(p->local_ops.size() > 1000 && w.tiny_first <= (gran ? 8 : 2) && (gran || w.n_tiny == 0) &&
                      w.n_large + w.n_skew > 0,
                  "%c %d: %zu tiles -> %lld shaped ops, %lld pieces", op, m, p->local_ops.size(),
                  (long long)w.tiny_first, (long long)w.n_tiny);
            std::printf("merge %c %d: %zu tiles -> %lld op(s), %lld large / %lld skew sub-tiles\n", op, m,
                        p->local_ops.size(), (long long)w.tiny_first, (long long)w.n_large, (long long)w.n_skew);
        }
    // tiles that continue each other along s only (each strip's destination elsewhere): merged
    // they would be 24-wide strips, a third of the fp64 sub-tile, so they stay apart
    std::vector<costa_tile_op_t> strips;
    const int64_t lda = 4096;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 170; ++j) {
            costa_tile_op_t o{};
            o.src = (uint64_t(1) << 40) + uint64_t((j * 24 * lda + i * 24) * 8);
            o.dst = (uint64_t(1) << 41) + (uint64_t(i) << 32) + uint64_t(j * 24 * 8);
            o.nf = o.ns = 24;
            o.lds = int32_t(lda);
            o.ldd = 8192;
            o.flags = COSTA_TILE_TRANSPOSE | COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
            o.order = uint32_t(strips.size() + 1);
            strips.push_back(o);
        }
    std::vector<costa_tile_op_t> ord;
    std::vector<uint64_t> work;
    const work_split w = build_work(COSTA_DOUBLE, strips, ord, work, list_unpack);
    CHECK(w.tiny_first == 0 && w.n_large == 0, "thin strips: %lld shaped ops", (long long)w.tiny_first);
    std::printf("merge: %zu tiles continuing along s only -> %lld shaped ops, %lld pieces\n", strips.size(),
                (long long)w.tiny_first, (long long)w.n_tiny);
    return true;
}

// the sub-tiled work items cover their ops exactly: every (op, sub-tile) of ordered[0, tiny_first)
// once, each class's items naming only its own ops, whatever order the sorts (hint, destination
// address, 128 KiB panels, XCD groups of the skew shape) left them in; with panels, the items walk
// the destination panel by panel
static bool check_cover(const std::string& name, costa_dtype_t dt, const std::vector<costa_tile_op_t>& ops,
                        bool expect_panels = false) {
    std::vector<costa_tile_op_t> ord;
    std::vector<uint64_t> work;
    const work_split w = build_work(dt, ops, ord, work, list_local);
    shape_dims sh;
    tile_shapes(dt, w.tr_shape, &sh);
    const int64_t E = int64_t(dtype_size(dt));
    CHECK(w.n_cblock == 0, "%lld destination-block groups (run with COSTA_CBLOCK=0)", (long long)w.n_cblock);
    CHECK(int64_t(work.size()) == w.n_large + w.n_medium + w.n_skew, "%zu work items, split %lld + %lld + %lld",
          work.size(), (long long)w.n_large, (long long)w.n_medium, (long long)w.n_skew);
    const int bfs[3][2] = {{w.sq ? sh.bf_q : sh.bf, w.sq ? sh.bs_q : sh.bs},
                           {w.med_sq ? sh.bf_s : sh.bf_m, w.med_sq ? sh.bs_s : sh.bs_m},
                           {w.skew_wide ? sh.bf_kw : sh.bf_k, w.skew_wide ? sh.bs_kw : sh.bs_k}};
    const int64_t ends[3] = {w.n_large, w.n_large + w.n_medium, w.n_large + w.n_medium + w.n_skew};
    std::vector<int> cls(size_t(w.tiny_first), -1);
    std::vector<std::vector<char>> seen(size_t(w.tiny_first));
    int64_t covered = 0, want = 0, panel_back = 0;
    for (int64_t i = 0; i < w.tiny_first; ++i) want += int64_t(ord[size_t(i)].nf) * ord[size_t(i)].ns;
    uint64_t last_panel = 0, lo = ~uint64_t(0);
    for (int64_t i = 0; i < w.tiny_first; ++i) lo = std::min(lo, ord[size_t(i)].dst);
    for (int64_t x = 0; x < int64_t(work.size()); ++x) {
        const int c = x < ends[0] ? 0 : x < ends[1] ? 1 : 2;
        const int bf = bfs[c][0], bs = bfs[c][1];
        CHECK(bf > 0 && bs > 0, "item %lld in class %d without a shape", (long long)x, c);
        const uint64_t i = work[size_t(x)] >> 32, q = work[size_t(x)] & 0xFFFFFFFFull;
        CHECK(int64_t(i) < w.tiny_first, "item %lld names op %llu past the shaped ops", (long long)x,
              (unsigned long long)i);
        const costa_tile_op_t& op = ord[size_t(i)];
        const uint64_t nbf = uint64_t((op.nf + bf - 1) / bf), n = nbf * uint64_t((op.ns + bs - 1) / bs);
        CHECK(cls[i] == -1 || cls[i] == c, "op %llu in two classes", (unsigned long long)i);
        cls[i] = c;
        if (seen[i].empty()) seen[i].assign(size_t(n), 0);
        CHECK(q < n && !seen[i][q], "op %llu sub-tile %llu (of %llu) twice or out of range", (unsigned long long)i,
              (unsigned long long)q, (unsigned long long)n);
        seen[i][q] = 1;
        const int64_t f0 = int64_t(q % nbf) * bf, s0 = int64_t(q / nbf) * bs;
        covered += std::min<int64_t>(bf, op.nf - f0) * std::min<int64_t>(bs, op.ns - s0);
        if (expect_panels && c == 0) {  // engine.cpp build_work: 128 KiB panels of destination rows
            const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
            const uint64_t e = (op.dst - lo) / uint64_t(E) +uint64_t(tr ? f0 * op.ldd + s0 : s0 * op.ldd + f0);
            const uint64_t panel = (e % uint64_t(op.ldd)) / uint64_t((int64_t(128) << 10) / E);
            panel_back += panel < last_panel;
            last_panel = panel;
        }
    }
    CHECK(covered == want, "sub-tiles cover %lld of %lld elements", (long long)covered, (long long)want);
    for (int64_t i = 0; i < w.tiny_first; ++i) CHECK(cls[size_t(i)] >= 0, "op %lld has no work item", (long long)i);
    CHECK(!expect_panels || panel_back == 0,"%lld steps back to an earlier panel", (long long)panel_back);
    std::printf("cover %s: %lld shaped ops -> %zu items (%lld large, %lld medium, %lld skew)%s\n", name.c_str(),
                (long long)w.tiny_first, work.size(), (long long)w.n_large, (long long)w.n_medium,
                (long long)w.n_skew, expect_panels ? ", panels" : "");
    return true;
}

// destination-block groups (engine.cpp cblock_groups): every group's ops tile its R x K range
// exactly once (ldd = R, inside the range, no element twice, one transform), and together with
// the shaped ops and the wavefront pieces every op of the list is covered exactly (by its hint)
static bool check_cblock(const std::string& name, costa_dtype_t dt, const std::vector<costa_tile_op_t>& ops,
                         list_kind kind, bool expect_groups) {
    std::vector<costa_tile_op_t> ord;
    std::vector<uint64_t> work;
    const work_split w = build_work(dt, ops, ord, work, kind);
    const int64_t E = int64_t(dtype_size(dt));
    const uint32_t vec_bits = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    CHECK(int64_t(work.size()) == w.n_large + w.n_medium + w.n_skew + w.n_cblock, "%zu work items", work.size());
    CHECK(!expect_groups || w.n_cblock > 0, "no destination-block group");
    std::map<uint32_t, int64_t> area;
    int64_t lds = 0, grouped = 0, first = INT64_MAX;
    uint64_t last = 0;
    for (int64_t x = w.n_large + w.n_medium + w.n_skew; x < int64_t(work.size()); ++x) {
        const uint64_t h = work[size_t(x)];
        CHECK(h < uint64_t(w.tiny_first), "group header %llu past the groups", (unsigned long long)h);
        first = std::min(first, int64_t(h));
        const costa_tile_op_t& hd = ord[size_t(h)];
        const int64_t R = hd.nf, K = hd.ns, n = int64_t(hd.src);
        // (a range off the 16-byte grid needs up to V - 1 more elements of whole vectors)
        CHECK(R > 0 && K > 0 && n >= 1 && hd.ldd == R && R * K + 16 / E - 1 <= cblock_max_elems(E),
              "group %lld shape", (long long)x);
        // destination order (with XCD column bands: inside each of the 8 slices of the kernel's sizes)
        const int64_t gi = x - (w.n_large + w.n_medium + w.n_skew), ng = w.n_cblock;
        const bool slice_start = w.cb_map == cb_xcd_bands &&
                                 (gi < (ng % 8) * (ng / 8 + 1) ? gi % (ng / 8 + 1) == 0
                                                               : ng / 8 > 0 && (gi - (ng % 8) * (ng / 8 + 1)) % (ng / 8) == 0);
        CHECK(slice_start || hd.dst >= last, "group %lld out of destination order", (long long)x);
        last = hd.dst;
        lds = std::max(lds, (R | 1) * K);
        std::vector<char> cov(size_t(R * K), 0);
        for (int64_t i = 0; i < n; ++i) {
            const costa_tile_op_t& op = ord[size_t(h) + 1 + size_t(i)];
            const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
            const int64_t run = tr ? op.ns : op.nf, runs = tr ? op.nf : op.ns;
            CHECK(op.ldd == R && (op.flags & ~vec_bits) == hd.flags && op.dst >= hd.dst, "group %lld op %lld", (long long)x,
                  (long long)i);
            const int64_t e = int64_t(op.dst - hd.dst) / E, r0 = e % R, c0 = e / R;
            CHECK(r0 + run <= R && c0 + runs <= K, "group %lld op %lld outside the range", (long long)x, (long long)i);
            for (int64_t c = c0; c < c0 + runs; ++c)
                for (int64_t r = r0; r < r0 + run; ++r) {
                    CHECK(!cov[size_t(c * R + r)], "group %lld: element (%lld, %lld) twice", (long long)x, (long long)r,
                          (long long)c);
                    cov[size_t(c * R + r)] = 1;
                }
            area[op.order] += int64_t(op.nf) * op.ns;
            grouped += int64_t(op.nf) * op.ns;
        }
        for (char v : cov) CHECK(v, "group %lld not covered", (long long)x);
    }
    CHECK(lds == w.cblock_lds, "LDS image %lld, split says %lld", (long long)lds, (long long)w.cblock_lds);
    for (int64_t i = 0; i < std::min<int64_t>(first, w.tiny_first); ++i) area[ord[size_t(i)].order] += int64_t(ord[size_t(i)].nf) * ord[size_t(i)].ns;
    for (int64_t i = w.tiny_first; i < w.tiny_first + w.n_tiny; ++i) area[ord[size_t(i)].order] += int64_t(ord[size_t(i)].nf) * ord[size_t(i)].ns;
    for (const auto& o : ops)
        CHECK(area[o.order] == int64_t(o.nf) * o.ns, "op %u covered %lld of %lld", o.order, (long long)area[o.order],
              (long long)(int64_t(o.nf) * o.ns));
    std::printf("cblock %s: %zu ops -> %lld groups holding %lld elements, %lld pieces, LDS %lld elements\n", name.c_str(),
                ops.size(), (long long)w.n_cblock, (long long)grouped, (long long)w.n_tiny, (long long)lds);
    return true;
}

// the destination-block groups' XCD chunk order (engine.hpp cblock_xcd_order) is a permutation of
// the launch, whatever its size
static bool check_xcd() {
    const std::string name = "xcd order";
    for (int64_t nb = 1; nb <= 4096; ++nb) {
        std::vector<char> seen(size_t(nb), 0);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t g = cblock_xcd_order(b, nb);
            CHECK(g >= 0 && g < nb && !seen[size_t(g)], "nb %lld, b %lld -> %lld", (long long)nb, (long long)b,
                  (long long)g);
            seen[size_t(g)] = 1;
        }
        // and so is the slice order (xcd_slice_order), XCD b mod 8 inside slice b mod 8
        std::vector<char> seen2(size_t(nb), 0);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t g = xcd_slice_order(b, nb);
            const int64_t x = b % 8, lo = x < nb % 8 ? x * (nb / 8 + 1) : (nb % 8) * (nb / 8 + 1) + (x - nb % 8) * (nb / 8);
            CHECK(g >= 0 && g < nb && !seen2[size_t(g)] && g >= lo && g < lo + nb / 8 + (x < nb % 8),
                  "slice order: nb %lld, b %lld -> %lld", (long long)nb, (long long)b, (long long)g);
            seen2[size_t(g)] = 1;
        }
    }
    return true;
}

static bool check_cblocks() {
    const int n = 16384;
    auto LA = layout(splits(0xC5A1, 8, 96, n), splits(0xC5A2, 8, 96, n), uint64_t(1) << 40);
    auto LC = layout(splits(0xC5A3, 16, 160, n), splits(0xC5A4, 16, 160, n), uint64_t(1) << 41);
    elayout a = erase(LA), c = erase(LC);
    for (char op : {'N', 'T'}) {
        auto p = plan_of(a, c, op, op == 'N' ? 1.f : -0.5f, op == 'N' ? 0.f : 2.f);
        if (!check_cblock(std::string("cfg5 ") + op, p->dtype, p->local_ops, list_local, true)) return false;
        if (!check_cblock(std::string("cfg5 unpack-list ") + op, p->dtype, p->local_ops, list_unpack, true)) return false;
        // every 8th op: the ranges are no longer covered, so no group forms
        std::vector<costa_tile_op_t> sub;
        for (size_t i = 0; i < p->local_ops.size(); i += 8) sub.push_back(p->local_ops[i]);
        if (!check_cblock(std::string("cfg5 sub-list ") + op, p->dtype, sub, list_local, false)) return false;
    }
    // C blocks of 200 x 200 fp64 (over the budget: cut into column bands) and blocks separated by
    // gaps, fed by 24 x 24 A blocks
    // (gap 3: every block after the first starts off the 16-byte grid, as in test_gpu_cblock.py)
    auto LA2 = layout<double>(splits(7, 20, 28, 2000), splits(8, 20, 28, 2000), uint64_t(1) << 40);
    auto LC2 = layout<double>(splits(9, 150, 250, 2000), splits(10, 150, 250, 2000), uint64_t(1) << 41, 3);
    elayout a2 = erase(LA2), c2 = erase(LC2);
    for (char op : {'N', 'T'}) {
        job j{&a2, &c2, op, {}};
        const double one = 1.0, zero = 0.0;
        std::memcpy(j.s.alpha.data(), &one, 8);
        std::memcpy(j.s.beta.data(), &zero, 8);
        auto p = make_plan({j}, 0, 1);
        if (!check_cblock(std::string("fp64 bands ") + op, p->dtype, p->local_ops, list_local, true)) return false;
    }
    return true;
}

template <typename T>
static std::unique_ptr<plan> square_plan(int m, int nb, int lld, char op) {
    auto A = block_cyclic_layout<T>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                    reinterpret_cast<T*>(uint64_t(1) << 40), lld, 'C', 0);
    auto C = block_cyclic_layout<T>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                    reinterpret_cast<T*>(uint64_t(1) << 42), lld, 'C', 0);
    elayout ea = erase(A), ec = erase(C);
    job j{&ea, &ec, op, {}};
    const T one = T(1), zero = T(0);
    std::memcpy(j.s.alpha.data(), &one, sizeof(T));
    std::memcpy(j.s.beta.data(), &zero, sizeof(T));
    return make_plan({j}, 0, 1);
}

// copies into destinations off the 64-byte grid cut at the granules (engine.cpp granule_split,
// run with COSTA_TUNING=1 COSTA_COPY_GRANULE=1): every destination element is written exactly once,
// from the source element of the same (row, column); the sub-tiled ops start every destination
// column on a 64-byte granule
template <typename T>
static bool check_granule_case(int m, int nb, int lda, int ldc, T beta) {
    const std::string name = "granule";
    const int64_t E = int64_t(sizeof(T));
    const uint64_t A0 = uint64_t(1) << 40, C0 = uint64_t(1) << 42;
    auto A = block_cyclic_layout<T>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0, reinterpret_cast<T*>(A0), lda, 'C', 0);
    auto C = block_cyclic_layout<T>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0, reinterpret_cast<T*>(C0), ldc, 'C', 0);
    elayout ea = erase(A), ec = erase(C);
    job j{&ea, &ec, 'N', {}};
    const T one = T(1);
    std::memcpy(j.s.alpha.data(), &one, sizeof(T));
    std::memcpy(j.s.beta.data(), &beta, sizeof(T));
    auto p = make_plan({j}, 0, 1);
    std::vector<costa_tile_op_t> ord;
    std::vector<uint64_t> work;
    const work_split w = build_work(p->dtype, p->local_ops, ord, work, list_local);
    std::vector<char> hit(size_t(ldc) * size_t(m), 0);
    int64_t aligned_ops = 0;
    auto walk = [&](const costa_tile_op_t& o) {
        CHECK(!(o.flags & COSTA_TILE_TRANSPOSE), "a copy became a transpose");
        for (int64_t s = 0; s < o.ns; ++s)
            for (int64_t f = 0; f < o.nf; ++f) {
                const int64_t ea_ = int64_t(o.src - A0) / E + s * o.lds + f;
                const int64_t ec_ = int64_t(o.dst - C0) / E + s * o.ldd + f;
                const int64_t i = ea_ % lda, jj = ea_ / lda;
                CHECK(i < m && jj < m && ec_ == i + jj * int64_t(ldc), "element (%lld, %lld) misplaced", (long long)i,
                      (long long)jj);
                CHECK(!hit[size_t(ec_)], "element (%lld, %lld) written twice", (long long)i, (long long)jj);
                hit[size_t(ec_)] = 1;
            }
        return true;
    };
    for (int64_t i = 0; i < w.tiny_first; ++i) {
        const costa_tile_op_t& o = ord[size_t(i)];
        if (!walk(o)) return false;
        // every sub-tiled op's destination columns start on a granule
        CHECK(o.dst % 64 == 0 && (uint64_t(o.ldd) * uint64_t(E)) % 64 == 0, "sub-tiled op %lld off the granules",
              (long long)i);
        ++aligned_ops;
    }
    for (int64_t i = w.tiny_first; i < w.tiny_first + w.n_tiny; ++i)
        if (!walk(ord[size_t(i)])) return false;
    int64_t n_hit = 0;
    for (char h : hit) n_hit += h;
    CHECK(n_hit == int64_t(m) * m, "%lld of %lld elements written", (long long)n_hit, (long long)int64_t(m) * m);
    CHECK(aligned_ops > 0, "no sub-tiled op");
    std::printf("granule E=%lld lda %d ldc %d: %lld sub-tiled ops (granule-aligned), %lld large items, %lld pieces\n",
                (long long)E, lda, ldc, (long long)aligned_ops, (long long)w.n_large, (long long)w.n_tiny);
    return true;
}

static bool check_granule() {
    for (int pad : {1, 2, 3, 8})
        if (!check_granule_case<double>(2048, 256, 2048, 2048 + pad, 0.0) ||
            !check_granule_case<double>(2048, 256, 2048 + pad, 2048 + pad, 2.0))
            return false;
    for (int pad : {1, 4, 8, 24})
        if (!check_granule_case<float>(2048, 256, 2048, 2048 + pad, 0.f) ||
            !check_granule_case<float>(2048, 200, 2048 + 3, 2048 + pad, 0.5f))
            return false;
    return check_granule_case<int>(2048, 256, 2048, 2051, 0);
}

static bool check_covers() {
    using z = std::complex<double>;
    struct g {
        const char* name;
        std::unique_ptr<plan> p;
        bool panels;
    };
    std::vector<g> gs;
    gs.push_back({"fp64 32768^2 256^2 'T'", square_plan<double>(32768, 256, 32768, 'T'), true});
    gs.push_back({"fp64 16384^2 256^2 'T'", square_plan<double>(16384, 256, 16384, 'T'), false});
    gs.push_back({"c128 32768^2 128^2 'T'", square_plan<z>(32768, 128, 32768, 'T'), true});
    gs.push_back({"c128 8192^2 80^2 'T' (merged)", square_plan<z>(8192, 80, 8192, 'T'), false});
    gs.push_back({"fp64 8192^2 100^2 'N' (merged)", square_plan<double>(8192, 100, 8192, 'N'), false});
    gs.push_back({"fp32 4096^2 256^2 'T' lld 4097 (skew)", square_plan<float>(4096, 256, 4097, 'T'), false});
    gs.push_back({"fp64 8192^2 32^2 'T' lld 8196 (skew)", square_plan<double>(8192, 32, 8196, 'T'), false});
    {
        // eight separate 32768 x 4096 column strips of A (no merging) into one 32768^2 C: 'T'
        // writes 256 KiB destination columns, walked in panels across the eight ops
        std::vector<int> rs{0, 32768}, cs;
        for (int j = 0; j <= 8; ++j) cs.push_back(4096 * j);
        auto A = layout<double>(rs, cs, uint64_t(1) << 40, 64);
        auto C = block_cyclic_layout<double>(32768, 32768, 32768, 32768, 1, 1, 32768, 32768, 1, 1, 'R', 0, 0,
                                             reinterpret_cast<double*>(uint64_t(1) << 42), 32768, 'C', 0);
        elayout ea = erase(A), ec = erase(C);
        job j{&ea, &ec, 'T', {}};
        const double one = 1.0, zero = 0.0;
        std::memcpy(j.s.alpha.data(), &one, 8);
        std::memcpy(j.s.beta.data(), &zero, 8);
        gs.push_back({"fp64 8 strips 32768 x 4096 'T'", make_plan({j}, 0, 1), true});
    }
    for (const auto& x : gs)
        if (!check_cover(x.name, x.p->dtype, x.p->local_ops, x.panels)) return false;
    const int n = 16384;
    auto LA = layout(splits(0xC5A1, 8, 96, n), splits(0xC5A2, 8, 96, n), uint64_t(1) << 40);
    auto LC = layout(splits(0xC5A3, 16, 160, n), splits(0xC5A4, 16, 160, n), uint64_t(1) << 41);
    elayout a = erase(LA), c = erase(LC);
    for (char op : {'N', 'T'}) {
        auto p = plan_of(a, c, op, 1.f, 0.f);
        if (!check_cover(std::string("cfg5 ") + op, p->dtype, p->local_ops)) return false;
    }
    return true;
}

// FNV-1a over the work lists of a set of geometries (cfg 5 'N' / 'T', cfg 2's 256^2 fp64 'T',
// cfg 4's 128^2 c128 'T' with alpha / beta, 24^2 fp32 blocks that merge, fp32 with lld 4097):
// `work_check digest` prints it, so that tests/test_work_lists.py can compare builds of the
// library under different environments
static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
static uint64_t digest_of(uint64_t h, const plan& p) {
    for (int kind = 0; kind < 3; ++kind) {
        const auto& ops = kind == 0 ? p.local_ops : kind == 1 ? p.pack_ops : p.unpack_ops;
        std::vector<costa_tile_op_t> ord;
        std::vector<uint64_t> work;
        const work_split w = build_work(p.dtype, ops, ord, work, kind == 0 ? list_local : kind == 1 ? list_pack : list_unpack);
        h = fnv(h, ord.data(), ord.size() * sizeof(costa_tile_op_t));
        h = fnv(h, work.data(), work.size() * sizeof(uint64_t));
        h = fnv(h, &w, sizeof(w));
    }
    return h;
}
static int digest() {
    uint64_t h = 0xcbf29ce484222325ull;
    const int n = 16384;
    auto LA = layout(splits(0xC5A1, 8, 96, n), splits(0xC5A2, 8, 96, n), uint64_t(1) << 40);
    auto LC = layout(splits(0xC5A3, 16, 160, n), splits(0xC5A4, 16, 160, n), uint64_t(1) << 41);
    elayout a = erase(LA), c = erase(LC);
    for (char op : {'N', 'T'}) h = digest_of(h, *plan_of(a, c, op, op == 'N' ? 1.f : -0.5f, op == 'N' ? 0.f : 2.f));
    {
        auto A = block_cyclic_layout<double>(n, n, 256, 256, 1, 1, n, n, 1, 1, 'R', 0, 0,
                                             reinterpret_cast<double*>(uint64_t(1) << 40), n, 'C', 0);
        auto C = block_cyclic_layout<double>(n, n, 256, 256, 1, 1, n, n, 1, 1, 'R', 0, 0,
                                             reinterpret_cast<double*>(uint64_t(1) << 41), n, 'C', 0);
        elayout ea = erase(A), ec = erase(C);
        job j{&ea, &ec, 'T', {}};
        const double one = 1.0, zero = 0.0;
        std::memcpy(j.s.alpha.data(), &one, 8);
        std::memcpy(j.s.beta.data(), &zero, 8);
        h = digest_of(h, *make_plan({j}, 0, 1));
    }
    {
        using z = std::complex<double>;
        const int m = 8192;
        auto A = block_cyclic_layout<z>(m, m, 128, 128, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                        reinterpret_cast<z*>(uint64_t(1) << 40), m, 'C', 0);
        auto C = block_cyclic_layout<z>(m, m, 128, 128, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                        reinterpret_cast<z*>(uint64_t(1) << 41), m, 'C', 0);
        elayout ea = erase(A), ec = erase(C);
        job j{&ea, &ec, 'T', {}};
        const z al(0.75, -0.5), be(1.25, 0.25);
        std::memcpy(j.s.alpha.data(), &al, 16);
        std::memcpy(j.s.beta.data(), &be, 16);
        h = digest_of(h, *make_plan({j}, 0, 1));
    }
    for (int lld : {4096, 4097}) {
        const int m = 4096, nb = lld == m ? 24 : 256;
        auto A = block_cyclic_layout<float>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                            reinterpret_cast<float*>(uint64_t(1) << 40), lld, 'C', 0);
        auto C = block_cyclic_layout<float>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                            reinterpret_cast<float*>(uint64_t(1) << 41), lld, 'C', 0);
        elayout ea = erase(A), ec = erase(C);
        for (char op : {'T', 'N'}) h = digest_of(h, *plan_of(ea, ec, op, 1.f, 0.f));
    }
    std::printf("digest %016llx\n", (unsigned long long)h);
    return 0;
}

// ---- `work_check strip`: the work lists of the strip kernel families (strip_work.hpp) against their
// rules, restated here.  Bytes a side must be aligned to for its VEC flag, per (source, destination)
// element size:
struct want_align {
    uint64_t es, ed, as, ad;
};
static const want_align kPairAlign[] = {{4, 8, 8, 16},  {8, 4, 16, 8}, {8, 16, 8, 16}, {16, 8, 16, 8},  // 2:1 pairs
                                        {2, 2, 8, 8},   {4, 2, 16, 8}, {2, 4, 8, 16},                   // half pairs
                                        {1, 1, 16, 16}, {4, 1, 16, 4}, {1, 4, 4, 16}};                  // FP8 pairs
static uint64_t scaled_align(uint64_t e) { return e == 1 ? 4 : e == 2 ? 8 : 16; }

template <typename Op>
static std::vector<Op> strip_ops(int bf, int bs, uint64_t es, uint64_t ed, int so, int d_o, bool tr) {
    const int shp[][2] = {{1, 1}, {3, 5}, {bf + 1, bs + 1}, {2 * bf - 1, 7}, {7, 2 * bs - 1}, {0, 3}};
    std::vector<Op> v;
    uint64_t sa = 4096, da = uint64_t(1) << 24;
    for (auto& s : shp) {
        Op t{};
        costa_tile_op_t& op = tile_of(t);
        op.nf = s[0], op.ns = s[1];
        op.lds = (s[0] + 15) / 16 * 16 + (so & 1);
        op.ldd = ((tr ? s[1] : s[0]) + 15) / 16 * 16 + (d_o & 1);
        op.src = sa + so * es, op.dst = da + d_o * ed;
        op.flags = (tr ? COSTA_TILE_TRANSPOSE : 0u) | COSTA_TILE_VEC_SRC;  // (a stale flag: must be recomputed)
        v.push_back(t);
        sa += 1 << 20, da -= 1 << 20;  // destinations descend: dst_order has something to sort
    }
    return v;
}

// what every list must satisfy; `listed(op, sub)`: 0 = not listed, 1 = listed, 2 = listed as whole
template <typename Op, typename Listed>
static bool check_strip(const std::string& name, const std::vector<Op>& in, const std::vector<Op>& ord,
                        const std::vector<uint64_t>& work, const strip_list& l, int bf, int bs, uint64_t es,
                        uint64_t ed, uint64_t as, uint64_t ad, uint64_t src_base, uint64_t dst_base, int shift,
                        Listed listed, bool dst_order) {
    auto fail = [&](const char* what) { std::printf("FAIL strip %s: %s\n", name.c_str(), what); return false; };
    std::map<uint64_t, int> want;  // item -> times seen
    size_t k = 0;
    bool tr = false;
    for (const Op& t : in) {
        const costa_tile_op_t& op = tile_of(t);
        if (op.nf <= 0 || op.ns <= 0) continue;
        const int64_t nbf = (op.nf + bf - 1) / bf, nbs = (op.ns + bs - 1) / bs;
        bool any = false;
        for (int64_t q = 0; q < nbf * nbs; ++q)
            if (const int c = listed(t, int(q % nbf), int(q / nbf))) {
                want[uint64_t(k) << 32 | uint64_t(q) << shift | uint64_t(shift && c == 2)] = 0;
                any = true;
            }
        if (!any) continue;
        if (k >= ord.size()) return fail("an op is missing");
        const costa_tile_op_t& o = tile_of(ord[k]);
        const uint32_t vec = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
        if (o.src != op.src || o.dst != op.dst || o.nf != op.nf || o.ns != op.ns || (o.flags & ~vec) != (op.flags & ~vec))
            return fail("ordered is not the listed ops in list order");
        const bool vs = (src_base + op.src) % as == 0 && (uint64_t(op.lds) * es) % as == 0;
        const bool vd = (dst_base + op.dst) % ad == 0 && (uint64_t(op.ldd) * ed) % ad == 0;
        if (bool(o.flags & COSTA_TILE_VEC_SRC) != vs || bool(o.flags & COSTA_TILE_VEC_DST) != vd)
            return fail("a VEC flag off the alignment table");
        tr |= bool(op.flags & COSTA_TILE_TRANSPOSE);
        ++k;
    }
    if (k != ord.size() || l.n_items != int64_t(work.size()) || l.any_transpose != tr) return fail("list summary");
    uint64_t last_key = 0, last_item = 0;
    for (size_t x = 0; x < work.size(); ++x) {
        auto it = want.find(work[x]);
        if (it == want.end() || it->second++) return fail("an item not expected, or listed twice");
        uint64_t key = 0;
        if (dst_order) {
            const costa_tile_op_t& o = tile_of(ord[size_t(work[x] >> 32)]);
            const int64_t q = int64_t((work[x] & 0xFFFFFFFFull) >> shift), nbf = (o.nf + bf - 1) / bf;
            const int64_t f0 = q % nbf * bf, s0 = q / nbf * bs;
            key = o.dst + uint64_t(o.flags & COSTA_TILE_TRANSPOSE ? f0 * o.ldd + s0 : s0 * o.ldd + f0) * ed;
        }
        if (x && (key < last_key || (key == last_key && work[x] < last_item)))
            return fail(dst_order ? "not in destination-address order (stable)" : "not in list order");
        last_key = key, last_item = work[x];
    }
    if (work.size() != want.size()) return fail("a sub-tile is missing");
    return true;
}

static bool check_strips() {
    const costa_dtype_t all[] = {COSTA_FLOAT, COSTA_DOUBLE, COSTA_CFLOAT, COSTA_CDOUBLE, COSTA_INT32,
                                 COSTA_HALF,  COSTA_BFLOAT16, COSTA_FP8_E4M3, COSTA_FP8_E5M2};
    auto every = [](const auto&, int, int) { return 1; };
    for (costa_dtype_t a : all)
        for (costa_dtype_t c : all)
            for (int tr = 0; tr < 2; ++tr)
                for (int so = 0; so < 4; ++so)
                    for (int d_o = 0; d_o < 4; ++d_o) {
                        const uint64_t es = dtype_size(a), ed = dtype_size(c), sb = so == 3 ? 2 : 0, db = d_o == 2 ? 4 : 0;
                        const std::string name = std::string(dtype_name(a)) + " -> " + dtype_name(c) + (tr ? " T" : " N") +
                                                 " +" + std::to_string(so) + " +" + std::to_string(d_o);
                        std::vector<uint64_t> work;
                        int bf, bs;
                        if (convertible(a, c)) {
                            const want_align* w = nullptr;
                            for (const want_align& x : kPairAlign)
                                if (x.es == es && x.ed == ed) w = &x;
                            if (!w) return false;
                            convert_subtile(a, c, &bf, &bs);
                            const auto ops = strip_ops<costa_tile_op_t>(bf, bs, es, ed, so, d_o, tr);
                            std::vector<costa_tile_op_t> ord;
                            const strip_list l = build_convert_work(a, c, ops, sb, db, ord, work);
                            if (!check_strip("pair " + name, ops, ord, work, l, bf, bs, es, ed, w->as, w->ad, sb, db, 0, every, false))
                                return false;
                        }
                        if (scaled_pair(a, c))
                            for (int by_dst = 0; by_dst < 2; ++by_dst) {
                                scaled_subtile(a, c, &bf, &bs);
                                auto ops = strip_ops<costa_scaled_op_t>(bf, bs, es, ed, so, d_o, tr);
                                ops[1].op.dst = ops[3].op.dst;  // (a tie for the stable sort)
                                std::vector<costa_scaled_op_t> ord;
                                const strip_list l = build_scaled_work(a, c, ops, sb, db, ord, work, by_dst);
                                if (!check_strip("scaled " + name, ops, ord, work, l, bf, bs, es, ed, scaled_align(es),
                                                 scaled_align(ed), sb, db, 0, every, by_dst))
                                    return false;
                            }
                        if (a == c && !dtype_is_half(a) && !dtype_is_fp8(a))
                            for (int le = 0; le < 2; ++le)
                                for (int diag : {-(1 << 30), -130, -64, -3, 0, 1, 5, 63, 70, 1 << 30}) {
                                    tri_subtile(a, &bf, &bs);
                                    auto ops = strip_ops<costa_tri_op_t>(bf, bs, es, ed, so, d_o, tr);
                                    for (auto& t : ops) t.diag = diag, t.op.flags |= le ? COSTA_TRI_LE : 0u;
                                    // brute force: a sub-tile is listed when an element of it is kept,
                                    // whole when all are
                                    auto scan = [&](const costa_tri_op_t& t, int i, int j) {
                                        int64_t kept = 0, n = 0;
                                        for (int s = j * bs; s < std::min(t.op.ns, (j + 1) * bs); ++s)
                                            for (int f = i * bf; f < std::min(t.op.nf, (i + 1) * bf); ++f, ++n)
                                                kept += le ? s - f <= diag : s - f >= diag;
                                        return kept == 0 ? 0 : kept == n ? 2 : 1;
                                    };
                                    std::vector<costa_tri_op_t> ord;
                                    const strip_list l = build_tri_work(a, ops, sb, db, ord, work);
                                    if (!check_strip("tri " + name + (le ? " LE " : " GE ") + std::to_string(diag), ops, ord,
                                                     work, l, bf, bs, es, ed, 16, 16, sb, db, 1, scan, false))
                                        return false;
                                }
                    }
    return true;
}

// ---- `work_check rounds`: the exchange round of every pack and unpack op (engine.cpp
// exchange_round_of_ops / _tri / _scaled) against the rule, restated here: a peer's package of n units
// moves in the parts round_range(n, E, R, r); a pack op belongs to the round that sends its FIRST unit
// (everything a round sends is packed by then), an unpack op to the round that brings its LAST unit
// (everything it reads has arrived); no op reaches into another peer's package.  A wrong round is a
// race on the GPU that the emulated-rank tests cannot see (their package is whole before any unpack).
static void set_one_zero(job& j, costa_dtype_t compute) {
    const double d1 = 1.0, d0 = 0.0;
    const float f1 = 1.f, f0 = 0.f;
    if (compute == COSTA_DOUBLE) {
        std::memcpy(j.s.alpha.data(), &d1, 8);
        std::memcpy(j.s.beta.data(), &d0, 8);
    } else {
        std::memcpy(j.s.alpha.data(), &f1, 4);
        std::memcpy(j.s.beta.data(), &f0, 4);
    }
}

// `rank`'s part of an m x n matrix in bm x bn blocks dealt over a pm x pn rank grid
template <typename T>
static elayout cyclic(int m, int n, int bm, int bn, int pm, int pn, int rank, uint64_t base) {
    return erase(block_cyclic_layout<T>(m, n, bm, bn, 1, 1, m, n, pm, pn, 'R', 0, 0, reinterpret_cast<T*>(base), m, 'C',
                                        rank));
}

// ... of a matrix in ragged blocks whose owners favour the low ranks (packages of very different sizes)
static elayout ragged(const std::vector<int>& rs, const std::vector<int>& cs, int n_ranks, int rank, uint64_t seed,
                      uint64_t base) {
    const int nr = int(rs.size()) - 1, nc = int(cs.size()) - 1;
    std::mt19937_64 r(seed);
    std::vector<int> own(size_t(nr) * size_t(nc));
    for (int& o : own) {
        const int x = int(r() % 16);
        o = x < 9 ? 0 : x < 15 ? 1 % n_ranks : 2 % n_ranks;
    }
    std::vector<block_t> blocks;
    uint64_t off = 0;
    for (int i = 0; i < nr; ++i)
        for (int j = 0; j < nc; ++j) {
            if (own[size_t(i) * size_t(nc) + size_t(j)] != rank) continue;
            const int rows = rs[size_t(i) + 1] - rs[size_t(i)], cols = cs[size_t(j) + 1] - cs[size_t(j)];
            blocks.push_back({reinterpret_cast<void*>(base + 4 * off), rows, i, j});
            off += (uint64_t(rows) * uint64_t(cols) + 63) / 64 * 64;
        }
    return erase(custom_layout<float>(nr, nc, rs.data(), cs.data(), own.data(), int(blocks.size()), blocks.data(), 'C'));
}

struct round_tally {
    int64_t split = 0, whole = 0;  // peer packages at or above round_min_bytes() / below it
    int64_t pack = 0, unpack = 0, tri = 0, scaled = 0;
};

static bool check_rounds_of(const std::string& name, const plan& p, int R, round_tally& n) {
    const size_t E = pkg_unit_size(p.pkg_dtype);
    std::vector<int> pr, ur, tr, sr;
    exchange_round_of_ops(p, R, pr, ur);
    exchange_round_of_tri(p, R, tr);
    exchange_round_of_scaled(p, R, sr);
    CHECK(pr.size() == p.pack_ops.size() && ur.size() == p.unpack_ops.size() && tr.size() == p.unpack_tri.size() &&
              sr.size() == p.unpack_scaled.size(),
          "a round per op: %zu / %zu / %zu / %zu", pr.size(), ur.size(), tr.size(), sr.size());
    // an op over package units [first, first + units) of the buffer laid out by displs / counts, assigned
    // round r: inside one peer's package, the unit that decides (first or last) in r's range
    auto one = [&](const char* what, size_t i, const std::vector<int64_t>& displs, const std::vector<int64_t>& counts,
                   int64_t first, int64_t units, bool by_last, int r) {
        CHECK(units > 0 && r >= 0 && r < R, "%s op %zu: %lld units, round %d of %d", what, i, (long long)units, r, R);
        size_t q = 0;
        while (q < counts.size() && !(first >= displs[q] && first < displs[q] + counts[q])) ++q;
        CHECK(q < counts.size(), "%s op %zu: unit %lld in no peer's package", what, i, (long long)first);
        CHECK(first + units <= displs[q] + counts[q], "%s op %zu straddles the packages of peers %zu and %zu", what, i, q,
              q + 1);
        int64_t lo, hi;
        round_range(counts[q], E, R, r, lo, hi);
        const int64_t at = (by_last ? first + units - 1 : first) - displs[q];
        CHECK(at >= lo && at < hi, "%s op %zu: its %s unit %lld of peer %zu is outside round %d's [%lld, %lld)", what, i,
              by_last ? "last" : "first", (long long)at, q, r, (long long)lo, (long long)hi);
        return true;
    };
    for (size_t i = 0; i < p.pack_ops.size(); ++i) {  // (a packed package's pack ops are byte ops: nf x ns units)
        const costa_tile_op_t& op = p.pack_ops[i];
        if (!one("pack", i, p.send_displs, p.send_counts, int64_t(op.dst / E), int64_t(op.nf) * op.ns, false, pr[i]))
            return false;
    }
    for (size_t i = 0; i < p.unpack_ops.size(); ++i) {
        const costa_tile_op_t& op = p.unpack_ops[i];
        if (!one("unpack", i, p.recv_displs, p.recv_counts, int64_t(op.src / E), int64_t(op.nf) * op.ns, true, ur[i]))
            return false;
    }
    for (size_t i = 0; i < p.unpack_tri.size(); ++i) {
        const costa_tile_op_t& op = p.unpack_tri[i].op;
        if (!one("tri unpack", i, p.recv_displs, p.recv_counts, int64_t(op.src / E), int64_t(op.nf) * op.ns, true, tr[i]))
            return false;
    }
    for (size_t i = 0; i < p.unpack_scaled.size(); ++i) {  // (nf x ns elements: of a packed package, their bytes)
        const costa_tile_op_t& op = p.unpack_scaled[i].op;
        if (!one("scaled unpack", i, p.recv_displs, p.recv_counts, int64_t(op.src / E),
                 pkg_units(p.pkg_dtype, int64_t(op.nf) * op.ns), true, sr[i]))
            return false;
    }
    if (R > 1) {
        for (const auto* counts : {&p.send_counts, &p.recv_counts})
            for (int64_t c : *counts)
                if (c > 0) ++(size_t(c) * E >= round_min_bytes() ? n.split : n.whole);
        n.pack += int64_t(pr.size()), n.unpack += int64_t(ur.size()), n.tri += int64_t(tr.size());
        n.scaled += int64_t(sr.size());
    }
    return true;
}

static bool check_rounds() {
    const std::string name = "rounds";
    const uint64_t A0 = uint64_t(1) << 40, C0 = uint64_t(1) << 42;
    round_tally n;
    // the plans of every rank of a case, checked for the library's rounds and for a single one
    auto run = [&](const std::string& what, int n_ranks, auto make_job) {
        for (int rank = 0; rank < n_ranks; ++rank) {
            elayout a, c;
            job j = make_job(rank, a, c);
            j.A = &a, j.C = &c;
            const auto p = make_plan({j}, rank, n_ranks);
            for (int R : {exchange_rounds(), 1})
                if (!check_rounds_of(what + ", rank " + std::to_string(rank) + ", R = " + std::to_string(R), *p, R, n))
                    return false;
        }
        return true;
    };
    // block-cyclic pairs, fp64 4096^2: over 2 ranks 32 MiB per peer (moved in rounds), over 4 ranks 8 MiB (whole)
    for (int ranks : {2, 4})
        for (char op : {'N', 'T'})
            if (!run(std::string("cyclic ") + op + " over " + std::to_string(ranks), ranks, [&](int rank, elayout& a, elayout& c) {
                    a = cyclic<double>(4096, 4096, 128, 128, ranks / 2, 2, rank, A0);
                    c = cyclic<double>(4096, 4096, 96, 160, 2, ranks / 2, rank, C0);
                    job j;
                    j.trans = op;
                    set_one_zero(j, COSTA_DOUBLE);
                    return j;
                }))
                return false;
    // a ragged custom pair over 3 ranks, fp32 6000 x 5000, owners skewed: packages of both kinds
    if (!run("ragged custom", 3, [&](int rank, elayout& a, elayout& c) {
            a = ragged(splits(0xA1, 40, 300, 6000), splits(0xA2, 40, 300, 5000), 3, rank, 0xA3, A0);
            c = ragged(splits(0xC1, 60, 500, 6000), splits(0xC2, 60, 500, 5000), 3, rank, 0xC3, C0);
            job j;
            set_one_zero(j, COSTA_FLOAT);
            return j;
        }))
        return false;
    // a triangular job (edge tiles in unpack_tri), fp64 4096^2 over 2 ranks
    for (char uplo : {'U', 'L'})
        if (!run(std::string("triangular ") + uplo, 2, [&](int rank, elayout& a, elayout& c) {
                a = cyclic<double>(4096, 4096, 128, 128, 1, 2, rank, A0);
                c = cyclic<double>(4096, 4096, 96, 160, 2, 1, rank, C0);
                job j;
                j.uplo = uplo;
                j.k = uplo == 'U' ? 3 : -5;
                set_one_zero(j, COSTA_DOUBLE);
                return j;
            }))
            return false;
    // a scaled fp32 -> e4m3 job (every unpack op in unpack_scaled; the package holds fp32), 4096^2 over 2 ranks
    if (!run("scaled FLOAT -> FP8_E4M3", 2, [&](int rank, elayout& a, elayout& c) {
            a = cyclic<float>(4096, 4096, 128, 128, 1, 2, rank, A0);
            c = cyclic<fp8_e4m3_bits>(4096, 4096, 96, 160, 2, 1, rank, C0);
            job j;
            j.scaled = true;
            set_one_zero(j, COSTA_FLOAT);
            return j;
        }))
        return false;
    // a packed FP4 job (the package holds A's bytes, two elements each: pkg_units), 16384^2 over 2 ranks: 32 MiB
    // per peer; 'T' too, and 2048^2 (below the threshold)
    for (int m : {16384, 2048})
        for (char op : {'N', 'T'})
            if (!run(std::string("MX FP4_E2M1 -> FLOAT ") + op + " " + std::to_string(m), 2, [&](int rank, elayout& a, elayout& c) {
                    a = cyclic<fp8_e4m3_bits>(m, m, 256, 256, 1, 2, rank, A0);  // the geometry; then two elements a byte
                    a.dtype = COSTA_FP4_E2M1;
                    for (eblock& b : a.blocks) b.data = reinterpret_cast<char*>(A0 + (reinterpret_cast<uintptr_t>(b.data) - A0) / 2);
                    c = cyclic<float>(m, m, 192, 320, 2, 1, rank, C0);
                    job j;
                    j.trans = op;
                    j.scaled = j.mx = true;
                    set_one_zero(j, COSTA_FLOAT);
                    return j;
                }))
                return false;
    CHECK(n.split > 0 && n.whole > 0, "%lld packages moved in rounds, %lld whole: both branches must run",
          (long long)n.split, (long long)n.whole);
    CHECK(n.pack > 0 && n.unpack > 0 && n.tri > 0 && n.scaled > 0, "ops checked: %lld pack, %lld unpack, %lld tri, %lld scaled",
          (long long)n.pack, (long long)n.unpack, (long long)n.tri, (long long)n.scaled);
    std::printf("rounds: R = %d, %lld packages in rounds, %lld whole; %lld pack, %lld unpack, %lld tri, %lld scaled ops\n",
                exchange_rounds(), (long long)n.split, (long long)n.whole, (long long)n.pack, (long long)n.unpack,
                (long long)n.tri, (long long)n.scaled);
    return true;
}

// ---- `work_check extents`: work lists of ops whose leading dimensions put part of them past 2^32
// bytes / 2^31 elements (tests/test_extents_plan_cpu.py).  A plan of an m x n block-cyclic pair with
// leading dimensions lda / ldc: every record of the executor's ordered list (sub-tiled ops, the ops of
// destination-block groups, wavefront pieces), walked element by element in 64-bit arithmetic, moves
// op(A)(i, j) to C(i, j), every element exactly once; the sub-tile items cover their ops exactly
// (check_cover) where no group formed.
template <typename T>
static std::unique_ptr<plan> rect_plan(int m, int n, int nb, int64_t lda, int64_t ldc, char op, uint64_t A0, uint64_t C0) {
    const int am = op == 'N' ? m : n, an = op == 'N' ? n : m;
    auto A = block_cyclic_layout<T>(am, an, nb, nb, 1, 1, am, an, 1, 1, 'R', 0, 0, reinterpret_cast<T*>(A0), int(lda), 'C', 0);
    auto C = block_cyclic_layout<T>(m, n, nb, nb, 1, 1, m, n, 1, 1, 'R', 0, 0, reinterpret_cast<T*>(C0), int(ldc), 'C', 0);
    elayout ea = erase(A), ec = erase(C);
    job j{&ea, &ec, op, {}};
    const T one = T(1), zero = T(0);
    std::memcpy(j.s.alpha.data(), &one, sizeof(T));
    std::memcpy(j.s.beta.data(), &zero, sizeof(T));
    return make_plan({j}, 0, 1);
}

struct extent_lists {
    work_split w;
    std::vector<costa_tile_op_t> ord;
    std::vector<uint64_t> work;
};

template <typename T>
static bool check_extent_case(const std::string& name, int m, int n, int nb, int64_t lda, int64_t ldc, char op,
                              extent_lists* out = nullptr) {
    const int64_t E = int64_t(sizeof(T));
    const uint64_t A0 = uint64_t(1) << 40, C0 = uint64_t(1) << 44;
    auto p = rect_plan<T>(m, n, nb, lda, ldc, op, A0, C0);
    extent_lists l;
    l.w = build_work(p->dtype, p->local_ops, l.ord, l.work, list_local);
    const work_split& w = l.w;
    std::vector<char> header(l.ord.size(), 0), hit(size_t(m) * size_t(n), 0);
    for (int64_t x = w.n_large + w.n_medium + w.n_skew; x < int64_t(l.work.size()); ++x) header[size_t(l.work[size_t(x)])] = 1;
    int64_t far = 0;
    for (size_t x = 0; x < l.ord.size(); ++x) {
        if (header[x]) continue;
        const costa_tile_op_t& o = l.ord[x];
        const bool tr = o.flags & COSTA_TILE_TRANSPOSE;
        CHECK(tr == (op != 'N') && o.src >= A0 && o.dst >= C0 && (o.src - A0) % uint64_t(E) == 0 && (o.dst - C0) % uint64_t(E) == 0,
              "record %zu: flags or base", x);
        for (int64_t s = 0; s < o.ns; ++s)
            for (int64_t f = 0; f < o.nf; ++f) {
                const int64_t ea_ = int64_t(o.src - A0) / E + s * int64_t(o.lds) + f;
                const int64_t ec_ = int64_t(o.dst - C0) / E + (tr ? f * int64_t(o.ldd) + s : s * int64_t(o.ldd) + f);
                const int64_t ai = ea_ % lda, aj = ea_ / lda, i = ec_ % ldc, j = ec_ / ldc;
                CHECK(i < m && j < n && (tr ? (ai == j && aj == i) : (ai == i && aj == j)),
                      "record %zu: C(%lld, %lld) from A(%lld, %lld)", x, (long long)i, (long long)j, (long long)ai, (long long)aj);
                CHECK(!hit[size_t(j) * size_t(m) + size_t(i)], "C(%lld, %lld) written twice", (long long)i, (long long)j);
                hit[size_t(j) * size_t(m) + size_t(i)] = 1;
                far = std::max(far, std::max(ea_, ec_));
            }
    }
    int64_t n_hit = 0;
    for (char h : hit) n_hit += h;
    CHECK(n_hit == int64_t(m) * n, "%lld of %lld elements written", (long long)n_hit, (long long)int64_t(m) * n);
    CHECK(far * E >= (int64_t(1) << 32), "nothing past 2^32 bytes (the case is not stretched)");
    if (w.n_cblock == 0 && !check_cover("extents " + name, p->dtype, p->local_ops)) return false;
    std::printf("extents %s: %zu records, %lld large + %lld medium + %lld skew items, %lld groups, %lld pieces, "
                "last element %lld\n", name.c_str(), l.ord.size(), (long long)w.n_large, (long long)w.n_medium,
                (long long)w.n_skew, (long long)w.n_cblock, (long long)w.n_tiny, (long long)far);
    if (out) *out = std::move(l);
    return true;
}

// ... and of any layout pair: every non-header record of the executor's ordered list walked element by
// element, the (destination address, source address) pairs sorted and compared with `want` (the closed
// form of the pair, sorted by destination address)
using addr_pair = std::pair<uint64_t, uint64_t>;
static bool check_extent_pairs(const std::string& name, const plan& p, int64_t E, std::vector<addr_pair> want,
                               bool want_groups, bool want_medium) {
    extent_lists l;
    l.w = build_work(p.dtype, p.local_ops, l.ord, l.work, list_local);
    const work_split& w = l.w;
    CHECK(!want_groups || (w.n_cblock > 0 && w.n_tiny > 0), "%lld groups, %lld pieces: both wanted", (long long)w.n_cblock,
          (long long)w.n_tiny);
    CHECK(!want_medium || w.n_medium >= 4096, "%lld medium items", (long long)w.n_medium);
    std::vector<char> header(l.ord.size(), 0);
    for (int64_t x = w.n_large + w.n_medium + w.n_skew; x < int64_t(l.work.size()); ++x) header[size_t(l.work[size_t(x)])] = 1;
    std::vector<addr_pair> got;
    got.reserve(want.size());
    uint64_t lo = ~uint64_t(0), hi = 0;
    for (size_t x = 0; x < l.ord.size(); ++x) {
        if (header[x]) continue;
        const costa_tile_op_t& o = l.ord[x];
        const bool tr = o.flags & COSTA_TILE_TRANSPOSE;
        for (int64_t s = 0; s < o.ns; ++s)
            for (int64_t f = 0; f < o.nf; ++f) {
                const uint64_t sa = o.src + uint64_t((s * int64_t(o.lds) + f) * E);
                got.push_back({o.dst + uint64_t((tr ? f * int64_t(o.ldd) + s : s * int64_t(o.ldd) + f) * E), sa});
                lo = std::min(lo, sa), hi = std::max(hi, sa);
            }
    }
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    CHECK(got.size() == want.size(), "%zu elements moved, the matrix has %zu", got.size(), want.size());
    for (size_t x = 0; x < got.size(); ++x)
        CHECK(got[x] == want[x], "element %zu: %#llx <- %#llx, expected %#llx <- %#llx", x, (unsigned long long)got[x].first,
              (unsigned long long)got[x].second, (unsigned long long)want[x].first, (unsigned long long)want[x].second);
    uint64_t dlo = ~uint64_t(0), dhi = 0;
    for (const auto& g : got) dlo = std::min(dlo, g.first), dhi = std::max(dhi, g.first);
    CHECK(std::max(hi - lo, dhi - dlo) >= (uint64_t(1) << 32), "nothing past 2^32 bytes (the case is not stretched)");
    // the groups' own invariants (each group's ops tile its range exactly once; check_cblock)
    if (w.n_cblock > 0 && !check_cblock("extents " + name, p.dtype, p.local_ops, list_local, true)) return false;
    if (w.n_cblock == 0 && !check_cover("extents " + name, p.dtype, p.local_ops)) return false;
    std::printf("extents %s: %zu records, %lld large + %lld medium + %lld skew items, %lld groups, %lld pieces\n", name.c_str(),
                l.ord.size(), (long long)w.n_large, (long long)w.n_medium, (long long)w.n_skew, (long long)w.n_cblock,
                (long long)w.n_tiny);
    return true;
}

// block (bi, bj)'s first element of layout()'s buffer, in elements (its blocks one after another)
static std::vector<uint64_t> layout_offsets(const std::vector<int>& rs, const std::vector<int>& cs, uint64_t gap) {
    std::vector<uint64_t> at;
    uint64_t off = 0;
    for (size_t i = 0; i + 1 < rs.size(); ++i)
        for (size_t j = 0; j + 1 < cs.size(); ++j) {
            at.push_back(off);
            off += (uint64_t(rs[i + 1] - rs[i]) * uint64_t(cs[j + 1] - cs[j]) + 63) / 64 * 64 + gap;
        }
    return at;
}

static std::unique_ptr<plan> float_plan(const elayout& a, const elayout& c, char op) { return plan_of(a, c, op, 1.f, 0.f); }

// destination-block groups and wavefront pieces fed from a source whose pitch is stretched: small
// A blocks (block-cyclic, lda = 7158279) tiling the compact blocks of a ragged custom C
static bool check_extent_groups(char op) {
    const int m = 300, n = 400;
    const int64_t lda = 7158279, E = 4;
    const uint64_t A0 = uint64_t(1) << 40, C0 = uint64_t(1) << 44;
    std::vector<int> rs = splits(21, 16, 60, m), cs = splits(22, 16, 60, n);
    rs.insert(rs.begin() + 1, 3);  // a lone strip of 3 rows: its blocks stay wavefront pieces
    const int am = op == 'N' ? m : n, an = op == 'N' ? n : m;
    auto A = block_cyclic_layout<float>(am, an, 24, 24, 1, 1, am, an, 1, 1, 'R', 0, 0, reinterpret_cast<float*>(A0), int(lda), 'C', 0);
    auto C = layout<float>(rs, cs, C0, 4);
    elayout ea = erase(A), ec = erase(C);
    auto p = float_plan(ea, ec, op);
    const std::vector<uint64_t> at = layout_offsets(rs, cs, 4);
    std::vector<addr_pair> want;
    for (size_t bi = 0; bi + 1 < rs.size(); ++bi)
        for (size_t bj = 0; bj + 1 < cs.size(); ++bj)
            for (int j = cs[bj]; j < cs[bj + 1]; ++j)
                for (int i = rs[bi]; i < rs[bi + 1]; ++i) {
                    const uint64_t d = at[bi * (cs.size() - 1) + bj] + uint64_t(j - cs[bj]) * uint64_t(rs[bi + 1] - rs[bi]) + uint64_t(i - rs[bi]);
                    const uint64_t sidx = op == 'N' ? uint64_t(j) * uint64_t(lda) + uint64_t(i) : uint64_t(i) * uint64_t(lda) + uint64_t(j);
                    want.push_back({C0 + d * E, A0 + sidx * E});
                }
    return check_extent_pairs(std::string("groups fp32 ragged C, stretched A ") + op, *p, E, std::move(want), true, false);
}

// the medium class: 65 x 64 separate 48 x 48 fp32 blocks of A (no two continue each other) transposed
// into a block-cyclic C of pitch 1400000: 4160 aligned transposing ops below the large class
static bool check_extent_medium() {
    const int nbr = 64, nbc = 65, b = 48;  // A is 3072 x 3120, C 3120 x 3072
    const int64_t ldc = 1400000, E = 4;
    const uint64_t A0 = uint64_t(1) << 40, C0 = uint64_t(1) << 44;
    std::vector<int> rs, cs;
    for (int i = 0; i <= nbr; ++i) rs.push_back(b * i);
    for (int j = 0; j <= nbc; ++j) cs.push_back(b * j);
    auto A = layout<float>(rs, cs, A0, 64);
    const int m = b * nbc, n = b * nbr;
    auto C = block_cyclic_layout<float>(m, n, b, b, 1, 1, m, n, 1, 1, 'R', 0, 0, reinterpret_cast<float*>(C0), int(ldc), 'C', 0);
    elayout ea = erase(A), ec = erase(C);
    auto p = float_plan(ea, ec, 'T');
    const std::vector<uint64_t> at = layout_offsets(rs, cs, 64);
    std::vector<addr_pair> want;
    want.reserve(size_t(m) * size_t(n));
    for (int j = 0; j < n; ++j)      // C(i, j) = A(j, i)
        for (int i = 0; i < m; ++i) {
            const uint64_t s = at[size_t(j / b) * size_t(nbc) + size_t(i / b)] + uint64_t(i % b) * b + uint64_t(j % b);
            want.push_back({C0 + (uint64_t(j) * uint64_t(ldc) + uint64_t(i)) * E, A0 + s * E});
        }
    return check_extent_pairs("medium fp32 48^2 blocks 'T', ldc 1400000", *p, E, std::move(want), false, true);
}

static bool check_extents() {
    const std::string name = "extents";
    using z = std::complex<double>;
    // byte rule (fp64, c128) and element rule (fp32), aligned and odd pitches, 'N' and 'T'
    for (char op : {'N', 'T'}) {
        const std::string o(1, op);
        if (!check_extent_case<double>("fp64 24^2 aligned " + o, 300, 400, 24, 1792256, 1792000 + 256 * 3, op)) return false;
        if (!check_extent_case<double>("fp64 128^2 odd " + o, 300, 400, 128, 1792257, 1792003, op)) return false;
        if (!check_extent_case<float>("fp32 24^2 odd, 2^31 elements " + o, 300, 400, 24, 7158279, 7158281, op)) return false;
        if (!check_extent_case<z>("c128 24^2 " + o, 300, 400, 24, 895232, 895233, op)) return false;
        // a compact block-cyclic target (one merged op: the large shape and pieces, no group)
        if (!check_extent_case<float>("fp32 24^2 compact C " + o, 300, 400, 24, 7158279, 300, op)) return false;
        if (!check_extent_groups(op)) return false;
    }
    if (!check_extent_medium()) return false;
    // granule_split gives up once max(lds, ldd) * 64 > INT32_MAX (its parts' pitch p * ld must fit an
    // int): just below, a copy into an odd pitch is cut at the granules (records of pitch p * ld);
    // above, every record keeps the op's own pitch
    for (int64_t ld : {int64_t(33554431), int64_t(33554433)}) {
        extent_lists l;
        if (!check_extent_case<float>("granule " + std::to_string(ld), 300, 64, 300, ld, ld, 'N', &l)) return false;
        bool cut = false;
        for (const auto& o : l.ord) cut = cut || o.ldd > ld;
        CHECK(cut == (ld * 64 <= INT32_MAX), "granule bail-out: pitch %lld %s", (long long)ld, cut ? "cut" : "not cut");
        std::printf("granule bail-out: pitch %lld %s\n", (long long)ld, cut ? "cut at the granules" : "left whole");
    }
    // the destination-panel sort key has 16 bits for the panel index: ldd / panel < 2^16.  fp64 'T',
    // panels of 16384 rows: at ldd = 2^30 - 16384 the key fits (the items walk panel by panel), at
    // ldd = 2^30 it does not and the items stay in plain destination-address order
    for (int64_t ld : {(int64_t(1) << 30) - 16384, int64_t(1) << 30}) {
        extent_lists l;
        if (!check_extent_case<double>("panel " + std::to_string(ld), 40000, 128, 40000, 128, ld, 'T', &l)) return false;
        shape_dims sh;
        tile_shapes(COSTA_DOUBLE, true, &sh);
        const int bf = l.w.sq ? sh.bf_q : sh.bf, bs = l.w.sq ? sh.bs_q : sh.bs;
        int64_t back = 0;
        uint64_t last = 0;
        for (int64_t x = 0; x < l.w.n_large; ++x) {
            const costa_tile_op_t& o = l.ord[size_t(l.work[size_t(x)] >> 32)];
            const int64_t q = int64_t(l.work[size_t(x)] & 0xFFFFFFFFull), nbf = (o.nf + bf - 1) / bf;
            const uint64_t at = o.dst + uint64_t(((q % nbf) * bf * int64_t(o.ldd) + (q / nbf) * bs) * 8);
            back += at < last;
            last = at;
        }
        const bool fits = ld / 16384 < 65536;
        CHECK(l.w.n_large > 1 && (back > 0) == fits, "panel key fallback: ldd %lld, %lld steps back in address order",
              (long long)ld, (long long)back);
        std::printf("panel key fallback: ldd %lld %s\n", (long long)ld, fits ? "panel order" : "plain address order");
    }
    // strip lists (converting, scaled, edge-tile) of one 300 x 260 op with stretched pitches: every
    // sub-tile once, VEC flags by the table, dst_order by 64-bit destination addresses
    auto every = [](const auto&, int, int) { return 1; };
    for (int tr = 0; tr < 2; ++tr) {
        std::vector<uint64_t> work;
        int bf, bs;
        auto one_op = [&](auto t, int64_t lds, int64_t ldd) {
            costa_tile_op_t& op = tile_of(t);
            op.nf = 300, op.ns = 260, op.lds = int32_t(lds), op.ldd = int32_t(ldd);
            op.src = 4096, op.dst = uint64_t(1) << 24;
            op.flags = tr ? COSTA_TILE_TRANSPOSE : 0u;
            return std::vector<decltype(t)>{t, t};
        };
        {
            convert_subtile(COSTA_DOUBLE, COSTA_FLOAT, &bf, &bs);
            auto ops = one_op(costa_tile_op_t{}, 2753324, 5506604);
            ops[1].dst += 64;
            std::vector<costa_tile_op_t> ord;
            const strip_list l = build_convert_work(COSTA_DOUBLE, COSTA_FLOAT, ops, 0, 0, ord, work);
            if (!check_strip("extents pair", ops, ord, work, l, bf, bs, 8, 4, 16, 8, 0, 0, 0, every, false)) return false;
        }
        for (int by_dst = 0; by_dst < 2; ++by_dst) {
            scaled_subtile(COSTA_FP8_E4M3, COSTA_FP8_E4M3, &bf, &bs);
            auto ops = one_op(costa_scaled_op_t{}, 22026412, 22026416);
            ops[1].op.dst -= 1 << 20;
            std::vector<costa_scaled_op_t> ord;
            const strip_list l = build_scaled_work(COSTA_FP8_E4M3, COSTA_FP8_E4M3, ops, 0, 0, ord, work, by_dst);
            if (!check_strip("extents scaled", ops, ord, work, l, bf, bs, 1, 1, 4, 4, 0, 0, 0, every, by_dst)) return false;
        }
        {
            tri_subtile(COSTA_DOUBLE, &bf, &bs);
            auto ops = one_op(costa_tri_op_t{}, 2753324, 2753326);
            for (auto& t : ops) t.diag = -(1 << 30);
            std::vector<costa_tri_op_t> ord;
            const strip_list l = build_tri_work(COSTA_DOUBLE, ops, 0, 0, ord, work);
            auto whole = [](const auto&, int, int) { return 2; };
            if (!check_strip("extents tri", ops, ord, work, l, bf, bs, 8, 8, 16, 16, 0, 0, 1, whole, false)) return false;
        }
    }
    // the limits are refusals: an op of more sub-tiles than a work item names
    {
        costa_tile_op_t t{};
        t.nf = t.ns = t.lds = t.ldd = INT32_MAX;
        int refused = 0;
        std::vector<uint64_t> work;
        try {
            std::vector<costa_tile_op_t> ord;
            build_convert_work(COSTA_DOUBLE, COSTA_FLOAT, {t}, 0, 0, ord, work);
        } catch (const error& e) { refused += e.code == COSTA_ERR_ARG && std::string(e.what()).find("list too long") != std::string::npos; }
        try {
            std::vector<costa_scaled_op_t> ord;
            costa_scaled_op_t st{};
            st.op = t;
            build_scaled_work(COSTA_FLOAT, COSTA_FLOAT, {st}, 0, 0, ord, work, false);
        } catch (const error& e) { refused += e.code == COSTA_ERR_ARG && std::string(e.what()).find("list too long") != std::string::npos; }
        for (uint32_t fl : {0u, uint32_t(COSTA_TILE_TRANSPOSE), uint32_t(COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST)}) {
            try {
                std::vector<costa_tile_op_t> ord;
                t.flags = fl | (COSTA_SCALE_ALPHA << COSTA_SCALE_SHIFT);
                build_work(COSTA_DOUBLE, {t}, ord, work, list_local);
            } catch (const error& e) { refused += e.code == COSTA_ERR_ARG && std::string(e.what()).find("tile too large") != std::string::npos; }
        }
        // ... and one that passes 2^32 sub-tiles far from INT32_MAX
        t.nf = t.ns = t.lds = t.ldd = 1 << 28;
        for (uint32_t fl : {0u, uint32_t(COSTA_TILE_TRANSPOSE | COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST)}) {
            try {
                std::vector<costa_tile_op_t> ord;
                t.flags = fl | (COSTA_SCALE_ALPHA << COSTA_SCALE_SHIFT);
                build_work(COSTA_DOUBLE, {t}, ord, work, list_local);
            } catch (const error& e) { refused += e.code == COSTA_ERR_ARG && std::string(e.what()).find("tile too large") != std::string::npos; }
        }
        CHECK(refused == 7, "strip / plain limits: %d of 7 lists refused with COSTA_ERR_ARG", refused);
        std::printf("strip and plain limits: 7 of 7 refused\n");
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "extents") {
        if (!check_extents()) return 1;
        std::printf("ok\n");
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "digest") return digest();
    if (argc > 1 && std::string(argv[1]) == "rounds") {
        if (!check_rounds()) return 1;
        std::printf("ok\n");
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "strip") {
        if (!check_strips()) return 1;
        std::printf("ok\n");
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "time") {  // build_work on cfg 5's 'N' list (host cost)
        const int n = 16384;
        auto LA = layout(splits(0xC5A1, 8, 96, n), splits(0xC5A2, 8, 96, n), uint64_t(1) << 40);
        auto LC = layout(splits(0xC5A3, 16, 160, n), splits(0xC5A4, 16, 160, n), uint64_t(1) << 41);
        elayout a = erase(LA), c = erase(LC);
        auto p = plan_of(a, c, 'N', 1.f, 0.f);
        std::vector<costa_tile_op_t> ord;
        std::vector<uint64_t> work;
        build_work(p->dtype, p->local_ops, ord, work, list_local);
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < 5; ++k) build_work(p->dtype, p->local_ops, ord, work, list_local);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / 5;
        std::printf("build_work cfg 5 'N' (%zu ops): %.2f ms\n", p->local_ops.size(), ms);
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "cover") {
        if (!check_covers()) return 1;
        std::printf("ok\n");
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "granule") {
        if (!check_granule()) return 1;
        std::printf("ok\n");
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "xcd") {
        if (!check_xcd()) return 1;
        std::printf("ok\n");
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "cblock") {
        if (!check_cblocks()) return 1;
        std::printf("ok\n");
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "merge") {
        if (!check_merge()) return 1;
        std::printf("ok\n");
        return 0;
    }
    const int n = 16384;
    auto LA = layout(splits(0xC5A1, 8, 96, n), splits(0xC5A2, 8, 96, n), uint64_t(1) << 40);
    auto LC = layout(splits(0xC5A3, 16, 160, n), splits(0xC5A4, 16, 160, n), uint64_t(1) << 41);
    elayout a = erase(LA), c = erase(LC);
    for (char op : {'N', 'T'}) {
        auto p = plan_of(a, c, op, op == 'N' ? 1.f : -0.5f, op == 'N' ? 0.f : 2.f);
        const std::set<uint32_t> shaped = expected_shaped(p->dtype, p->local_ops);
        if (!check_list(std::string("cfg5 ") + op, p->dtype, p->local_ops, shaped)) return 1;
        // one exchange round's share of a list: every 8th op (hints sparse)
        std::vector<costa_tile_op_t> sub;
        for (size_t i = 0; i < p->local_ops.size(); i += 8) sub.push_back(p->local_ops[i]);
        if (!check_list(std::string("cfg5 sub-list ") + op, p->dtype, sub, expected_shaped(p->dtype, sub)))
            return 1;
        // the same as a pack list (wavefront ops by source address)
        if (!check_list(std::string("cfg5 pack sub-list ") + op, p->dtype, sub, expected_shaped(p->dtype, sub, true), true))
            return 1;
    }
    // unaligned large ops: fp32 4096^2 'T' with lld = 4097 (columns 4-byte aligned only)
    for (int nb : {256, 1024}) {
        const int m = 4096, lld = m + 1;
        auto A = block_cyclic_layout<float>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                            reinterpret_cast<float*>(uint64_t(1) << 40), lld, 'C', 0);
        auto C = block_cyclic_layout<float>(m, m, nb, nb, 1, 1, m, m, 1, 1, 'R', 0, 0,
                                            reinterpret_cast<float*>(uint64_t(1) << 41), lld, 'C', 0);
        elayout ea = erase(A), ec = erase(C);
        auto p = plan_of(ea, ec, 'T', 1.f, 0.f);
        shape_dims sh;
        tile_shapes(COSTA_FLOAT, true, &sh);  // a transposing list
        // every op transposes into unaligned destination columns: the skew shape, whatever its size
        const std::set<uint32_t> expect = expected_shaped(p->dtype, p->local_ops);
        if (expect.size() != p->local_ops.size()) {
            std::printf("FAIL unaligned %d^2 blocks: %zu of %zu ops expected on the skew shape\n", nb,
                        expect.size(), p->local_ops.size());
            return 1;
        }
        if (!check_list("unaligned " + std::to_string(nb) + "^2 blocks", p->dtype, p->local_ops, expect))
            return 1;
    }
    std::printf("ok\n");
    return 0;
}
