// Kernels of scaled transforms for CDNA4 (gfx950): tile ops with row / column scale vectors,
//   C(i, j) = beta*C(i, j) + alpha * s_ij(op(A)(i, j)),     s_ij(x) = (x * r[i]) * c[j]
// (costa_hip.h, "scaled transforms").  An op is a costa_scaled_op_t: a costa_tile_op_t plus the
// target coordinates (row0, col0) of its source element (0, 0); with COSTA_SCALED_F_ROWS the op's
// fast index f walks target rows (i = row0 + f, j = col0 + s), else columns (i = row0 + s,
// j = col0 + f).  With w() the exact widening of a stored element to the compute type Tc (fp32; fp64
// for the DOUBLE pair), cvt() the conversion Tc -> C's type and g() tile_kernel's scale<Tc> (same
// branches, contraction off), an op computes for its source element x and old destination value y
//   cvt(g(s_ij(w(x)), w(y)))          (FLOAT -> H: w(cvt_H(x)) in place of w(x))
// in copy mode at dst(f, s), in transpose mode at dst(s, f).  The two products of s_ij are two
// separately rounded multiplications, r first; a NULL vector's product is skipped (wave-uniform).
// Scale kind BITCOPY is cvt(s_ij(w(x))): never a byte copy.  w() and cvt() are the device functions
// of half_kernel and fp8_kernel (tile_device.hpp).
//
// One kernel family, scaled_kernel<Es, Ed> (Es / Ed: the element codecs of the two sides, Tc =
// Ed::ct), driven like tri_kernel by a device array of ops and (op << 32) | sub-tile work items, with
// r and c as kernel arguments.  One workgroup of 256 threads runs one 64 x 64 sub-tile: the
// transposes are staged in the compute type (below), and 64 x 64 keeps that tile at 17 KiB (fp32) /
// 33 KiB (fp64) -- 128 x 128 would take 66 / 132 KiB, one workgroup per CU -- and a lane at 4 strips
// per side.  A lane's unit of work is a strip of 4 elements along the source's fast dimension: one
// dword on a 1-byte side, 8 bytes on a 2-byte side, 16 bytes on fp32, two 16-byte accesses on fp64,
// so consecutive lanes touch consecutive addresses on both sides.
//   copy mode       no LDS.  All source strips, all old destination strips (AXPBY) and the scale
//                   values are requested before the first use.  The scale along f (the destination's
//                   fast index) is one strip per lane, the same for its 4 passes; the scale along s
//                   one value per strip.  Every lane stores exactly the elements it loaded, so an op
//                   whose source and destination coincide (in-place equilibration) is safe; the
//                   data pointers carry no __restrict__.
//   transpose mode  the sub-tile is staged in LDS in the compute type for every pair, Q -> Q
//                   included: the scaling happens after the exchange (the strip load of the scale
//                   along the destination's fast index wants the transposed arrangement), in Tc, so
//                   fp8_kernel's byte staging would only move the widening behind the v_perm block
//                   transpose at the price of a second staging scheme; one scheme serves 14 pairs.
//                   Rows s, pitch 64 + 4 elements of fp32 (68 dwords) or 64 + 2 of fp64 (132 dwords):
//                   both are 4 mod 64 dwords, one 16-byte slot further per row.  Reads: lane l of a
//                   wavefront reads the strip of row l with ds_read_b128 (fp64: two), banks
//                   (a / 4) mod 64; each of the instruction's 16-lane groups holds 16 rows that
//                   differ mod 16, so their slots (17 l + q) mod 16 resp. (33 l + 2 q) mod 16 are all
//                   distinct: conflict-free.  Writes: ds_write_b128, banks (a / 4) mod 32, groups of
//                   8 consecutive lanes: fp32 lanes write 8 consecutive 16-byte strips of one row =
//                   32 distinct banks, conflict-free; fp64 lanes write two 16-byte halves 32 bytes
//                   apart, so lanes l and l + 4 of a group meet on a bank: 2-way on the fp64 writes
//                   (accepted: 2 x 4 write instructions per lane and sub-tile against 64 KiB of HBM
//                   traffic).  4 lanes then exchange their 4 x 4 block with lane_transpose (fp64:
//                   the low and high words separately), so every lane stores a strip along the
//                   destination's fast dimension; there the scale along s is the strip load and
//                   the scale along f one value per strip.
// Scale loads use the default cache policy (every sub-tile of a row or column band reads them
// again); the data uses non-temporal accesses as elsewhere.  A scale strip is one (fp64: two) 16-byte
// load where its address is 16-byte aligned (row0 / col0 + the sub-tile's origin a multiple of 4 on
// an aligned vector) and element-wise otherwise.
// Whole sub-tiles with both VEC flags take the FULL path, where every guard folds away; sub-tile
// remainders and sides off their strip's alignment (VEC flag clear) take the guarded, element-wise
// form of the same loads and stores: same values.  No scratch.
//
// amax outputs (costa_hip.h, "amax outputs"): the AMAX instantiations of scaled_kernel also update
// row_amax / col_amax, device arrays of U (the unsigned integer as wide as Tc), with
// absbits(w(x)) = the bits of the widened source value with the sign bit cleared, by an unsigned
// maximum; AMAX = false is the code above, unchanged.  The reduction uses the registers of the load
// phase, which holds the same elements in copy and transpose mode: lane t has strips x[k] at
// f = (t % 16) * 4 + e, s = t / 16 + 16 k.
//   along s   the maximum of a strip's 4 elements, then of the 16 lanes of its DPP row (row_ror 8, 4,
//             2, 1: every lane of the row ends with the row's maximum): one value per (t / 16, k),
//             stored to LDS by the row's first lane
//   along f   the maximum over k per element, then over the wavefront's 4 rows (two xor shuffles):
//             64 partial maxima per wavefront, stored to LDS by its first row; the 4 wavefronts'
//             partials meet in the update
// through one static LDS array of (4 + 1) x 64 U (1.25 KiB; fp64 2.5 KiB), which only these
// instantiations have, and ONE barrier: transpose mode's own, between staging and reading the tile;
// in copy mode one after the stores, so no wavefront waits for another before it stores.  Then
// wavefront 0 updates the 64 consecutive entries along s and wavefront 1 those along f with
// __hip_atomic_fetch_max (relaxed, agent scope, result unused): one 256-byte (fp64: 512-byte) wave
// instruction per vector and sub-tile, lanes past the sub-tile's tf / ts off.
// A lane first reads its entry with a plain load -- requested at the start, with the source loads,
// so that its latency is not added to the sub-tile's -- and skips the atomic when the entry is
// already >= its value: entries only grow, so a stale read can only cause a superfluous atomic,
// never a lost one; every sub-tile but the first few of a row or column band then issues none.  The
// zero tails of partial strips are harmless as values (0 is the least U) and never index a vector.
// A NULL vector's reduction is skipped (wave-uniform).  amax_kernel<Es> (costa_hip_layout_amax) is
// the copy-mode load phase and this reduction, and stores nothing.
// The mapping constants, codecs, strip loads and stores, staging helpers and DPP maxima live in
// strip_device.hpp, shared with mx_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>

#include "engine.hpp"
#include "strip_device.hpp"
#include "strip_launch.hpp"
#include "strip_work.hpp"
#include "tile_device.hpp"

#pragma clang fp contract(off)

namespace costa {
namespace engine {
namespace {

// a strip of a scale vector (default cache policy): 16-byte loads where the address allows, else
// element by element; elements past n stay 0 and are never used
template <typename C>
__device__ __forceinline__ void load_scale4(C (&out)[SV], const C* v, int n) {
#pragma unroll
    for (int k = 0; k < SV; ++k) out[k] = C(0);
    if (n >= SV && (reinterpret_cast<uintptr_t>(v) & 15u) == 0) {
        constexpr int NQ = int(sizeof(C)) * SV / 16;
        raw16 r[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) r[i] = *(reinterpret_cast<const raw16*>(v) + i);
        __builtin_memcpy(&out[0], &r[0], sizeof(C) * SV);
    } else {
#pragma unroll
        for (int k = 0; k < SV; ++k)
            if (k < n) out[k] = v[k];
    }
}

// ---- amax outputs: unsigned maximum of absbits over the load phase's registers ----
// entries of the reduction's LDS array: per wavefront its 64 partial maxima along f, then the 64
// maxima along s
constexpr int AMAX_LDS = SNW * SBF + SBS;
// the reduction is mapped to the default shape (a DPP row = the 16 lanes of one source column); a
// tuning build of another shape refuses amax vectors at the launch
constexpr bool AMAX_SHAPE = SLPC == 16 && SBF == 64 && SBS == 64 && SNW >= 2;

// The amax update of one sub-tile, in three steps every thread of the workgroup takes outside
// divergent control flow.  af (along f, tf entries) and as (along s, ts entries) point at the
// sub-tile's origin; either may be null (wave-uniform).
//   amax_begin    wavefront 0 (along s) and wavefront 1 (along f) read their 64 entries with plain
//                 loads, requested with the load phase's own loads: the value is only used to skip
//                 the atomic, so how old it is does not matter
//   amax_partial  the load phase's registers reduced into `red` (no barrier); elements outside
//                 tf x ts are 0 in x
//   amax_commit   after a barrier between amax_partial and it (the caller's): the two wavefronts
//                 update the entries their value would raise
template <typename U>
struct amax_out {
    U* v;   // this lane's entry (null: none)
    U cur;  // its value as read at the start
};
template <typename U, bool FULL>
__device__ __forceinline__ amax_out<U> amax_begin(U* af, U* as, int tf, int ts) {
    static_assert(AMAX_SHAPE, "the amax reduction is mapped to 64 x 64 sub-tiles of 256 threads");
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    amax_out<U> o{nullptr, U(0)};
    if (wave == 0 && as && (FULL || lane < ts)) o.v = as + lane;
    if (wave == 1 && af && (FULL || lane < tf)) o.v = af + lane;
    if (o.v) o.cur = *o.v;
    return o;
}
template <typename Es>
__device__ __forceinline__ void amax_partial(const strip<typename Es::st> (&x)[SPL], bool along_f, bool along_s,
                                             typename ubits<typename Es::ct>::type* red) {
    using U = typename ubits<typename Es::ct>::type;
    const int t = int(threadIdx.x), lane = t % 64, wave = t / 64;
    const int lf = (t % SLPC) * SV, c0 = t / SLPC;
    U a[SPL][SV];
#pragma unroll
    for (int k = 0; k < SPL; ++k)
#pragma unroll
        for (int e = 0; e < SV; ++e) a[k][e] = absbits(Es::widen(x[k].e[e]));
    if (along_s) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            U m = a[k][0];
#pragma unroll
            for (int e = 1; e < SV; ++e) m = umax(m, a[k][e]);
            m = row_max16(m);
            if (t % SLPC == 0) red[SNW * SBF + c0 + k * SCPP] = m;
        }
    }
    if (along_f) {
#pragma unroll
        for (int e = 0; e < SV; ++e) {
            U m = a[0][e];
#pragma unroll
            for (int k = 1; k < SPL; ++k) m = umax(m, a[k][e]);
            m = umax(m, U(__shfl_xor(m, 16)));
            m = umax(m, U(__shfl_xor(m, 32)));
            if (lane < SLPC) red[wave * SBF + lf + e] = m;
        }
    }
}
template <typename U>
__device__ __forceinline__ void amax_commit(const amax_out<U>& o, const U* red) {
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    if (!o.v) return;
    U m;
    if (wave == 0) {
        m = red[SNW * SBF + lane];
    } else {
        m = red[lane];
#pragma unroll
        for (int w = 1; w < SNW; ++w) m = umax(m, red[w * SBF + lane]);
    }
    if (m > o.cur) (void)__hip_atomic_fetch_max(o.v, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One sub-tile.  FULL: a whole 64 x 64 sub-tile with both VEC flags, every guard folds away.
// AMAX: ra / ca (row_amax / col_amax, either may be null) are updated from the load phase and `red`
// is the reduction's LDS array; else all three are unused.
template <typename Es, typename Ed, bool FULL, bool AMAX>
__device__ __forceinline__ void run_scaled(const costa_scaled_op_t& sop, int f0, int s0, int tf_, int ts_,
                                           const char* src_base, char* dst_base, typename Ed::ct alpha,
                                           typename Ed::ct beta, const typename Ed::ct* rs,
                                           const typename Ed::ct* cs, typename Ed::ct* tile,
                                           typename ubits<typename Ed::ct>::type* ra,
                                           typename ubits<typename Ed::ct>::type* ca,
                                           typename ubits<typename Ed::ct>::type* red) {
    using C = typename Ed::ct;
    using Ss = typename Es::st;
    using Sd = typename Ed::st;
    static_assert(std::is_same<typename Es::ct, C>::value, "one compute type");
    constexpr int P = sshape<C>::P;
    const costa_tile_op_t& op = sop.op;
    const int tf = FULL ? SBF : tf_;
    const int ts = FULL ? SBS : ts_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const bool vd = FULL || (flags & COSTA_TILE_VEC_DST);
    const int64_t lds = op.lds, ldd = op.ldd;
    // the vectors indexed along f and along s, at the sub-tile's origin (wave-uniform)
    const bool frow = flags & COSTA_SCALED_F_ROWS;
    const C* vf = frow ? rs : cs;
    const C* vsl = frow ? cs : rs;
    if (vf) vf += int64_t(frow ? sop.row0 : sop.col0) + f0;
    if (vsl) vsl += int64_t(frow ? sop.col0 : sop.row0) + s0;
    // s_ij(x) = (x * r[i]) * c[j]: two rounded products, r first; a NULL vector is skipped
    auto sx = [&](C x, C fv, C sv) {
        if (frow) {
            if (vf) x = x * fv;
            if (vsl) x = x * sv;
        } else {
            if (vsl) x = x * sv;
            if (vf) x = x * fv;
        }
        return x;
    };
    const Ss* src = reinterpret_cast<const Ss*>(src_base + op.src) + int64_t(s0) * lds + f0;

    // ---- load phase: lane -> (strip along f, column s); all loads issued first
    const int lf = (int(threadIdx.x) % SLPC) * SV;
    const int c0 = int(threadIdx.x) / SLPC;
    const int nf_lane = FULL ? SV : tf - lf;  // elements of this lane's strip inside the sub-tile
    strip<Ss> x[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = c0 + k * SCPP;
        x[k] = strip<Ss>{};
        if (FULL || (nf_lane > 0 && s < ts)) x[k] = load_strip(src + s * lds + lf, nf_lane, vs);
    }
    // amax outputs: the vectors indexed along f and along s at the sub-tile's origin; their entries
    // are requested with the source loads (amax_begin)
    using U = typename ubits<C>::type;
    [[maybe_unused]] amax_out<U> am{nullptr, U(0)};
    [[maybe_unused]] U* af = nullptr;
    [[maybe_unused]] U* as = nullptr;
    if constexpr (AMAX) {
        af = frow ? ra : ca;
        as = frow ? ca : ra;
        if (af) af += int64_t(frow ? sop.row0 : sop.col0) + f0;
        if (as) as += int64_t(frow ? sop.col0 : sop.row0) + s0;
        am = amax_begin<U, FULL>(af, as, tf, ts);
    }

    if (!(flags & COSTA_TILE_TRANSPOSE)) {
        // ---- copy mode: dst(f, s), no LDS
        Sd* dst = reinterpret_cast<Sd*>(dst_base + op.dst) + int64_t(s0) * ldd + f0;
        strip<Sd> y[SPL];  // beta != 0: every old value is requested before the first store
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int s = c0 + k * SCPP;
            y[k] = strip<Sd>{};
            if (kind == COSTA_SCALE_AXPBY && (FULL || (nf_lane > 0 && s < ts)))
                y[k] = load_strip(dst + s * ldd + lf, nf_lane, vd);
        }
        // the scale along f: one strip, the same for every pass; along s: one value per pass
        C fv[SV], sv[SPL];
#pragma unroll
        for (int e = 0; e < SV; ++e) fv[e] = C(0);
        if (vf && (FULL || nf_lane > 0)) load_scale4(fv, vf + lf, nf_lane);
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int s = c0 + k * SCPP;
            sv[k] = C(0);
            if (vsl && (FULL || s < ts)) sv[k] = vsl[s];
        }
        if constexpr (AMAX) amax_partial<Es>(x, af != nullptr, as != nullptr, red);
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int s = c0 + k * SCPP;
            if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
            strip<Sd> o;
#pragma unroll
            for (int e = 0; e < SV; ++e)
                o.e[e] = Ed::narrow(scale<C>(sx(Es::widen(x[k].e[e]), fv[e], sv[k]), Ed::widen(y[k].e[e]),
                                             kind, false, alpha, beta));
            store_strip(dst + s * ldd + lf, o, nf_lane, vd);
        }
        if constexpr (AMAX) {  // the update last: no wavefront waits for another before it stores
            __syncthreads();
            amax_commit(am, red);
        }
        return;
    }

    // ---- transpose mode: dst(s, f) through LDS, staged in the compute type
    Sd* dst = reinterpret_cast<Sd*>(dst_base + op.dst) + int64_t(f0) * ldd + s0;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    // store unit k of this lane: 64 s values of one f slot; after the lane exchange lane
    // (base + j) stores f = q*4 + j for s = sc*64 + base .. + 3
    const int j = lane & (SV - 1);
    auto unit = [&](int k, int& f, int& sb, int& n_s) {
        const int u = wave + SNW * k;
        const int sc = SBS == SSW ? 0 : u / SQG, q = SBS == SSW ? u : u % SQG;
        f = q * SV + j;
        sb = sc * SSW + (lane - j);
        n_s = FULL ? SV : ts - sb;
        return FULL || (f < tf && n_s > 0);
    };
    // beta != 0: the old destination values are requested now, with the source loads in flight
    strip<Sd> old[SPS];
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        int f, sb, n_s;
        old[k] = strip<Sd>{};
        if (kind == COSTA_SCALE_AXPBY && unit(k, f, sb, n_s)) old[k] = load_strip(dst + f * ldd + sb, n_s, vd);
    }
    // the scale along s (the destination's fast index): one strip per s chunk (a 64 x 64 sub-tile
    // has one: the same strip for every pass); along f: one value per pass
    constexpr int NSC = SBS / SSW;
    C sv[NSC][SV], fv[SPS];
#pragma unroll
    for (int sc = 0; sc < NSC; ++sc) {
        const int sb = sc * SSW + (lane - j);
#pragma unroll
        for (int e = 0; e < SV; ++e) sv[sc][e] = C(0);
        if (vsl && (FULL || ts - sb > 0)) load_scale4(sv[sc], vsl + sb, FULL ? SV : ts - sb);
    }
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        int f, sb, n_s;
        fv[k] = C(0);
        if (vf && unit(k, f, sb, n_s)) fv[k] = vf[f];
    }
    if constexpr (AMAX) amax_partial<Es>(x, af != nullptr, as != nullptr, red);  // (before the tile's barrier)
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = c0 + k * SCPP;
        if (FULL || (nf_lane > 0 && s < ts)) {  // partial strips: the tail is w(0), never stored
            C w[SV];
#pragma unroll
            for (int e = 0; e < SV; ++e) w[e] = Es::widen(x[k].e[e]);
            lds_put(tile + s * P + lf, w);
        }
    }
    __syncthreads();

    C y[SPS][SV];
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        const int u = wave + SNW * k;
        const int sc = SBS == SSW ? 0 : u / SQG, q = SBS == SSW ? u : u % SQG;
        const int s = sc * SSW + lane;
#pragma unroll
        for (int e = 0; e < SV; ++e) y[k][e] = C(0);
        if (FULL || (s < ts && q * SV < tf)) lds_get(y[k], tile + s * P + q * SV);
    }
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        transpose4(y[k], lane);  // (every lane takes part in the exchange)
        int f, sb, n_s;
        if (!unit(k, f, sb, n_s)) continue;
        // (SNW * k / SQG: compile-time; the units of one pass lie in one s chunk)
        constexpr int per_chunk = SQG / SNW;
        const C(&svk)[SV] = sv[SBS == SSW ? 0 : k / per_chunk];
        strip<Sd> o;
#pragma unroll
        for (int e = 0; e < SV; ++e)
            o.e[e] = Ed::narrow(scale<C>(sx(y[k][e], fv[k], svk[e]), Ed::widen(old[k].e[e]), kind, false,
                                         alpha, beta));
        store_strip(dst + f * ldd + sb, o, n_s, vd);
    }
    if constexpr (AMAX) amax_commit(am, red);
}

// AMAX: ra / ca are row_amax / col_amax (either may be null); else they are unused
template <typename Es, typename Ed, bool AMAX>
__global__ __launch_bounds__(SNT) void scaled_kernel(const costa_scaled_op_t* __restrict__ ops,
                                                     const uint64_t* __restrict__ work,
                                                     const char* src_base, char* dst_base,
                                                     const typename Ed::ct* __restrict__ scalars,
                                                     const typename Ed::ct* __restrict__ rs,
                                                     const typename Ed::ct* __restrict__ cs,
                                                     typename ubits<typename Ed::ct>::type* ra,
                                                     typename ubits<typename Ed::ct>::type* ca) {
    using C = typename Ed::ct;
    using U = typename ubits<C>::type;
    U* red = nullptr;
    if constexpr (AMAX) {
        __shared__ U amax_lds[AMAX_LDS];
        red = amax_lds;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    C* tile = reinterpret_cast<C*>(smem);
    // which sub-tile of which op (wave-uniform: scalar loads)
    const uint64_t w = work[blockIdx.x];
    const costa_scaled_op_t sop = ops[w >> 32];
    const costa_tile_op_t& op = sop.op;
    const uint32_t sub = uint32_t(w);
    const int nbf = (op.nf + SBF - 1) / SBF;
    const int f0 = int(sub % uint32_t(nbf)) * SBF;
    const int s0 = int(sub / uint32_t(nbf)) * SBS;
    const int tf = min(SBF, op.nf - f0);
    const int ts = min(SBS, op.ns - s0);
    const uint32_t slot = op.flags >> COSTA_SLOT_SHIFT;
    const C alpha = scalars[2 * slot];
    const C beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (tf == SBF && ts == SBS && (op.flags & vec_both) == vec_both)
        run_scaled<Es, Ed, true, AMAX>(sop, f0, s0, tf, ts, src_base, dst_base, alpha, beta, rs, cs, tile, ra,
                                       ca, red);
    else
        run_scaled<Es, Ed, false, AMAX>(sop, f0, s0, tf, ts, src_base, dst_base, alpha, beta, rs, cs, tile, ra,
                                        ca, red);
}

// costa_hip_layout_amax: the copy-mode load phase of scaled_kernel and its amax reduction over ops
// whose source side alone is used; nothing but the two vectors is written
template <typename Es>
__global__ __launch_bounds__(SNT) void amax_kernel(const costa_scaled_op_t* __restrict__ ops,
                                                   const uint64_t* __restrict__ work, const char* src_base,
                                                   typename ubits<typename Es::ct>::type* ra,
                                                   typename ubits<typename Es::ct>::type* ca) {
    using U = typename ubits<typename Es::ct>::type;
    using Ss = typename Es::st;
    __shared__ U red[AMAX_LDS];
    const uint64_t w = work[blockIdx.x];
    const costa_scaled_op_t sop = ops[w >> 32];
    const costa_tile_op_t& op = sop.op;
    const uint32_t sub = uint32_t(w);
    const int nbf = (op.nf + SBF - 1) / SBF;
    const int f0 = int(sub % uint32_t(nbf)) * SBF;
    const int s0 = int(sub / uint32_t(nbf)) * SBS;
    const int tf = min(SBF, op.nf - f0);
    const int ts = min(SBS, op.ns - s0);
    const bool vs = op.flags & COSTA_TILE_VEC_SRC;
    const bool frow = op.flags & COSTA_SCALED_F_ROWS;
    const int64_t lds = op.lds;
    U* af = frow ? ra : ca;
    U* as = frow ? ca : ra;
    if (af) af += int64_t(frow ? sop.row0 : sop.col0) + f0;
    if (as) as += int64_t(frow ? sop.col0 : sop.row0) + s0;
    const Ss* src = reinterpret_cast<const Ss*>(src_base + op.src) + int64_t(s0) * lds + f0;
    const int lf = (int(threadIdx.x) % SLPC) * SV;
    const int c0 = int(threadIdx.x) / SLPC;
    strip<Ss> x[SPL];
    amax_out<U> am;
    if (tf == SBF && ts == SBS && vs) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) x[k] = load_strip(src + (c0 + k * SCPP) * lds + lf, SV, true);
        am = amax_begin<U, true>(af, as, tf, ts);
    } else {
        const int nf_lane = tf - lf;
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int s = c0 + k * SCPP;
            x[k] = strip<Ss>{};
            if (nf_lane > 0 && s < ts) x[k] = load_strip(src + s * lds + lf, nf_lane, vs);
        }
        am = amax_begin<U, false>(af, as, tf, ts);
    }
    amax_partial<Es>(x, af != nullptr, as != nullptr, red);
    __syncthreads();
    amax_commit(am, red);
}

// the vectors of one launch: the scales (read) and the amax outputs (updated); any may be null
struct scaled_vecs {
    const void *rs, *cs;
    void *ra, *ca;
};

template <typename Es, typename Ed, bool AMAX>
void launch_inst(const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
                 const char* src_base, char* dst_base, const void* d_scalars, const scaled_vecs& v,
                 hipStream_t stream) {
    using C = typename Ed::ct;
    using U = typename ubits<C>::type;
    launch_strip<&scaled_kernel<Es, Ed, AMAX>, sshape<C>::lds_bytes>(
        "scaled", SNT, l, stream, d_ops, d_work, src_base, dst_base, static_cast<const C*>(d_scalars),
        static_cast<const C*>(v.rs), static_cast<const C*>(v.cs), static_cast<U*>(v.ra), static_cast<U*>(v.ca));
}

// the AMAX instantiation runs only where an amax vector is given
template <typename Es, typename Ed>
void launch_pair(const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
                 const char* src_base, char* dst_base, const void* d_scalars, const scaled_vecs& v,
                 hipStream_t stream) {
    if (!v.ra && !v.ca)
        launch_inst<Es, Ed, false>(d_ops, d_work, l, src_base, dst_base, d_scalars, v, stream);
    else if constexpr (AMAX_SHAPE)
        launch_inst<Es, Ed, true>(d_ops, d_work, l, src_base, dst_base, d_scalars, v, stream);
    else
        throw error(COSTA_ERR_ARG, "costa: this build's scaled sub-tile has no amax reduction");
}

// N: f16_t / bf16_t / e4m3_t / e5m2_t; ROUND: a FLOAT source is rounded to N first (the half pairs)
template <typename N, template <typename> class narrow_e, bool ROUND>
void launch_narrow(bool src_f, bool dst_f, const costa_scaled_op_t* d_ops,
                   const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                   const void* d_scalars, const scaled_vecs& v, hipStream_t s) {
    using src_e = typename std::conditional<ROUND, f32_via<N>, f32_e>::type;
    if (src_f)
        launch_pair<src_e, narrow_e<N>>(d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
    else if (dst_f)
        launch_pair<narrow_e<N>, f32_e>(d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
    else
        launch_pair<narrow_e<N>, narrow_e<N>>(d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
}

template <typename Es>
void launch_amax_of(const costa_scaled_op_t* d_ops, const uint64_t* d_work, int64_t n_items, void* ra,
                    void* ca, hipStream_t stream) {
    if constexpr (AMAX_SHAPE) {
        using U = typename ubits<typename Es::ct>::type;
        launch_strip<&amax_kernel<Es>, 0>("amax", SNT, strip_list{n_items, false}, stream, d_ops, d_work,
                                          static_cast<const char*>(nullptr), static_cast<U*>(ra), static_cast<U*>(ca));
    } else {
        throw error(COSTA_ERR_ARG, "costa: this build's scaled sub-tile has no amax reduction");
    }
}

}  // namespace

void scaled_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs) {
    if (!scaled_pair(src, dst))
        throw error(COSTA_ERR_ARG, std::string("costa: no scaled kernel for ") + dtype_name(src) + " -> " +
                                       dtype_name(dst));
    *bf = SBF;
    *bs = SBS;
}

void mx_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs) {
    if (!mx_pair(src, dst))
        throw error(COSTA_ERR_ARG, std::string("costa: no MX kernel for ") + dtype_name(src) + " -> " + dtype_name(dst));
    *bf = SBF;
    *bs = SBS;
}

strip_list build_scaled_work(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                             const std::vector<costa_scaled_op_t>& ops, uint64_t src_base,
                             uint64_t dst_base, std::vector<costa_scaled_op_t>& ordered,
                             std::vector<uint64_t>& work, bool dst_order) {
    // (a packed side of an MX pair: its strip of 4 is 2 bytes for FP4, and 3 bytes at any address for
    // FP6, where the flag is vacuous)
    const esize ES = elem_size(src_dtype), ED = elem_size(dst_dtype);
    strip_align al = strip_alignment(strip_family::scaled, std::max<uint64_t>(1, ES.qb / 4), std::max<uint64_t>(1, ED.qb / 4));
    if (dtype_is_fp4(src_dtype)) al.src = 2;
    if (dtype_is_fp4(dst_dtype)) al.dst = 2;
    if (dtype_is_fp6(src_dtype)) al.src = 1;
    if (dtype_is_fp6(dst_dtype)) al.dst = 1;
    for (const costa_scaled_op_t& t : ops) {  // (empty ops are skipped unchecked, as by the builder)
        if (t.op.nf <= 0 || t.op.ns <= 0) continue;
        if (t.op.lds < 0 || t.op.ldd < 0) throw error(COSTA_ERR_ARG, "costa: negative leading dimension");
        if (t.row0 < 0 || t.col0 < 0) throw error(COSTA_ERR_ARG, "costa: negative target coordinate");
    }
    return build_strip_work("scaled", ops, src_base, dst_base, SBF, SBS, ES, ED, al, ordered, work, all_listed(),
                            dst_order);
}

void launch_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* d_ops,
                   const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                   const void* d_scalars, const void* rs, const void* cs, void* row_amax, void* col_amax,
                   void* stream) {
    if (l.n_items <= 0) return;
    const scaled_vecs v{rs, cs, row_amax, col_amax};
    if (!scaled_pair(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, std::string("costa: no scaled kernel for ") + dtype_name(src_dtype) +
                                       " -> " + dtype_name(dst_dtype));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool src_f = src_dtype == COSTA_FLOAT, dst_f = dst_dtype == COSTA_FLOAT;
    const costa_dtype_t nt = src_f ? dst_dtype : src_dtype;  // the narrow type of a half / FP8 pair
    if (src_dtype == COSTA_DOUBLE)
        launch_pair<f64_e, f64_e>(d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
    else if (src_f && dst_f)
        launch_pair<f32_e, f32_e>(d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
    else if (nt == COSTA_HALF)
        launch_narrow<f16_t, h_e, true>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
    else if (nt == COSTA_BFLOAT16)
        launch_narrow<bf16_t, h_e, true>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
    else if (nt == COSTA_FP8_E4M3)
        launch_narrow<e4m3_t, q_e, false>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
    else
        launch_narrow<e5m2_t, q_e, false>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, v, s);
}

bool amax_dtype(costa_dtype_t t) {
    return t == COSTA_FLOAT || t == COSTA_DOUBLE || dtype_is_half(t) || dtype_is_fp8(t);
}

void launch_amax(costa_dtype_t dtype, const costa_scaled_op_t* d_ops, const uint64_t* d_work,
                 int64_t n_items, void* row_amax, void* col_amax, void* stream) {
    if (n_items <= 0) return;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
    case COSTA_FLOAT: launch_amax_of<f32_e>(d_ops, d_work, n_items, row_amax, col_amax, s); break;
    case COSTA_DOUBLE: launch_amax_of<f64_e>(d_ops, d_work, n_items, row_amax, col_amax, s); break;
    case COSTA_HALF: launch_amax_of<h_e<f16_t>>(d_ops, d_work, n_items, row_amax, col_amax, s); break;
    case COSTA_BFLOAT16: launch_amax_of<h_e<bf16_t>>(d_ops, d_work, n_items, row_amax, col_amax, s); break;
    case COSTA_FP8_E4M3: launch_amax_of<q_e<e4m3_t>>(d_ops, d_work, n_items, row_amax, col_amax, s); break;
    case COSTA_FP8_E5M2: launch_amax_of<q_e<e5m2_t>>(d_ops, d_work, n_items, row_amax, col_amax, s); break;
    default:
        throw error(COSTA_ERR_ARG, std::string("costa_hip_layout_amax: no amax of ") + dtype_name(dtype) +
                                       " (real floating-point element types only)");
    }
}

}  // namespace engine
}  // namespace costa
