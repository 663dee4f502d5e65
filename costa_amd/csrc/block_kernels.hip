// Kernels of block-scaled FP8 transforms for CDNA4 (gfx950): tile ops whose FP8 side carries one fp32
// scale per 1 x 128, 128 x 1 or 128 x 128 block of its matrix (costa_hip.h, "Block-scaled FP8
// transforms (fp32 scales)").  An op is a costa_scaled_op_t, as for scaled_kernel and mx_kernel: with
// COSTA_SCALED_F_ROWS the op's fast index f walks target rows (i = row0 + f, j = col0 + s), else
// columns.  Both scale tensors reach the kernel in TARGET coordinates (a block_side: the host has
// already swapped A's block shape and strides for a transposing job); a block extent is 1 or 128, so
// the block of an element is a shift of its coordinates.  With w() / cvt() the codecs of
// tile_device.hpp and g() tile_kernel's scale<float> (contraction off), an op computes per element
//   x = w(a) [* SA[block of a]]                   one rounded product
//   v = g(x, w(c_old))
//   dequantise (no c_scales): store v
//   quantise / requantise: per block of C, amax = unsigned max of the bits of |v|; exponent 255:
//     S = R = NaN; else amax_c = max(amax, 2^-40) and EXACT: S = amax_c / fmax, R = fmax / amax_c (two
//     correctly rounded divisions), POW2: E = block_E<Q>(amax_c, ceil), S = 2^(E-127), R = 2^(127-E);
//     q = cvt(clamp(v * R, -fmax, fmax)), SC[block] = S.
//
// Two kernels on the strip frame (strip_device.hpp, strip_work.hpp, strip_launch.hpp), 256 threads:
//   block_kernel<Es, f32_e, false>  dequantise: one 64 x 64 sub-tile per workgroup, the work items of
//                                   the scaled plan (build_scaled_work); mx_kernel<.., false> with an
//                                   fp32 scale load in place of the byte.
//   block_kernel<Es, Ed, true>      quantise / requantise: one 128 x 128 REGION of an op per workgroup
//                                   (build_block_work: the same builder on 128 x 128).  The planner
//                                   and costa_hip_execute_tiles_block_scaled guarantee that an op
//                                   starts on a multiple of C's block shape in target coordinates, and
//                                   regions start on multiples of 128 of the op, so every block of C
//                                   lies in ONE region (partial at the matrix edge): each scale float
//                                   is written once, by a plain vector store of the workgroup that owns
//                                   it.  No atomics, no second pass, no scratch memory.
// 128 x 128 regions were kept for all three block shapes (128 x 64 for the 1 x 128 shapes was not
// measured): one work list and one reduction frame serve every shape.
//
// Load phase: a region is NQ x NQ sub-tiles (NQ = 2; dequantise 1); sub-tile q = (qf, qs) lies at
// (64 qf, 64 qs) of the region.  Lane t holds of every sub-tile the strips x[q][k] at
// f = (t % 16) * 4 + e, s = t / 16 + 16 k: 16 strips of 4, 64 data VGPRs for a region.  The source
// strips, the old destination strips (dequantise, beta != 0) and the input scales are requested
// before the first use.  Input scales use the default cache policy (neighbouring strips, sub-tiles
// and regions read them again), data the non-temporal accesses of the strip loads and stores.  Where
// SA's blocks are 128 long along f and the origin along f is a multiple of 4 in target coordinates a
// strip lies inside one block and takes one load; otherwise each element indexes its own float.
// With beta = 0 (required with c_scales) v depends on x alone; the maxima are taken in the load
// arrangement, the same in copy and transpose mode, by the shape of C's block in (f, s):
//   128 x 1   (along f) a block is the 2 x 16 strips of one DPP row at one s: in-lane over the two
//             sub-tiles qf and the strip, then row_max16.  Registers only, no barrier; lane t % 16 == 0
//             stores the scale.
//   1 x 128   (along s) a block is one f over both qs, 4 passes and the 4 rows of all 4 wavefronts:
//             in-lane over qs and k, xor shuffles 16 and 32, then the wavefront's 128 partial maxima
//             go to LDS (red[wave][f], 512 words = 2 KiB) and meet after ONE barrier; lanes t < 16
//             store the scales.
//   128 x 128 in-lane over all 64 values, row_max16, xor shuffles 16 and 32, red[wave] (4 words), ONE
//             barrier; thread 0 stores the scale.
// S and R are then computed once per block and lane (8, 8 or 1 of them), the data is scaled, clamped
// in the load arrangement and stored: directly in copy mode; in transpose mode through the padded
// staged tile of scaled_kernel, ONE sub-tile at a time (barrier, 64 strips out, lane exchange, store,
// barrier before the tile is written again), so the workgroup stays within the 17 KiB the existing
// kernels stage.
// LDS words of `red` (bank = word mod 64).  Writes, 1 x 128: the first 16 lanes of a wavefront write 4
// consecutive words each, 64 consecutive words per (qf, element pass): conflict-free.  Reads after
// the barrier: 4 consecutive words per lane (16 bytes), the 16 lanes of a DPP row on 64 consecutive
// words and the 4 rows of the wavefront on the same words (broadcast), once per (wave, qf) slice.
// 128 x 128: one word per wavefront written by lane 0, 4 consecutive words read by every lane
// (broadcast).  The staged tile is scaled_kernel's: rows s, pitch 68 dwords, conflict-free as argued
// there.
// Whole regions (sub-tiles) with both VEC flags take the FULL path; remainders and unaligned sides the
// guarded one, where elements outside the region count as 0 in every maximum whatever alpha is.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "engine.hpp"
#include "strip_device.hpp"
#include "strip_launch.hpp"
#include "strip_work.hpp"
#include "tile_device.hpp"

#pragma clang fp contract(off)

namespace costa {
namespace engine {
namespace {

static_assert(SLPC == 16 && SBF == 64 && SBS == 64 && SNW == 4 && SPL == 4 && SPS == 4,
              "the block reduction is mapped to 64 x 64 sub-tiles of 256 threads");
constexpr int BLK = 128;                  // the long extent of a block = the region's edge
constexpr int BLK_RED = SNW * BLK;        // words of the reduction's LDS array
constexpr uint32_t BLK_EPS = 0x2B800000u; // 2^-40
constexpr uint32_t QNAN = 0x7FC00000u;

// the limits of the destination types (as mx_kernels.hip)
template <typename Q>
struct blim;
template <>
struct blim<e4m3_t> {
    static constexpr uint32_t emax = 8, fmax = 0x43E00000u;  // 448
};
template <>
struct blim<e5m2_t> {
    static constexpr uint32_t emax = 15, fmax = 0x47600000u;  // 57344
};
template <typename E>
struct bq_of {
    using type = e4m3_t;  // (unused for FLOAT destinations)
};
template <typename Q>
struct bq_of<q_e<Q>> {
    using type = Q;
};

// the MX rule of mx_kernels.hip (block_E with its pow2), for the POW2 scales
__device__ __forceinline__ float e8m0(uint32_t E) {
    return u2f(E == 0 ? 0x00400000u : E == 255 ? QNAN : E << 23);
}
template <typename Q>
__device__ __forceinline__ uint32_t mx_E(uint32_t amax, bool ceil) {
    const uint32_t e = amax >> 23;
    if (e == 255) return 255;
    uint32_t E = e > blim<Q>::emax ? e - blim<Q>::emax : 0u;
    if (ceil && E < 254 && u2f(amax) * e8m0(254 - E) > u2f(blim<Q>::fmax)) ++E;
    return E;
}
// S and R of a block from the bits of its amax
struct scale_pair {
    float S, R;
};
template <typename Q>
__device__ __forceinline__ scale_pair block_SR(uint32_t amax, bool p2) {
    if ((amax >> 23) == 255) return {u2f(QNAN), u2f(QNAN)};
    const uint32_t ac = umax(amax, BLK_EPS);
    if (p2) {
        const uint32_t E = mx_E<Q>(ac, true);  // (79 - emax <= E <= 247 - emax: both normal)
        return {u2f(E << 23), u2f((254 - E) << 23)};
    }
    const float a = u2f(ac), fm = u2f(blim<Q>::fmax);
    return {__fdiv_rn(a, fm), __fdiv_rn(fm, a)};  // correctly rounded; operands and results normal
}
// clamp(v * R): a NaN (R of a special block, or v) stays
template <typename Q>
__device__ __forceinline__ float quant(float v, float R) {
    const float t = v * R, fm = u2f(blim<Q>::fmax);
    return t > fm ? fm : t < -fm ? -fm : t;
}
__device__ __forceinline__ uint32_t wave_rows_max(uint32_t m) {
    m = umax(m, uint32_t(__shfl_xor(m, 16)));
    return umax(m, uint32_t(__shfl_xor(m, 32)));
}

// a scale tensor seen along (f, s) of an op
struct fs_side {
    float* data;
    int64_t f_stride, s_stride;
    int f_shift, s_shift;
    __device__ __forceinline__ int64_t at(int64_t F, int64_t S) const {
        return (F >> f_shift) * f_stride + (S >> s_shift) * s_stride;
    }
};
__device__ __forceinline__ fs_side along(const block_side& b, bool frow) {
    return frow ? fs_side{static_cast<float*>(b.data), b.row_stride, b.col_stride, b.row_shift, b.col_shift}
                : fs_side{static_cast<float*>(b.data), b.col_stride, b.row_stride, b.col_shift, b.row_shift};
}

template <typename Es, typename Ed, bool QUANT, bool FULL>
__device__ __forceinline__ void run_block(const costa_scaled_op_t& sop, int f0, int s0, int rf_, int rs_,
                                          const char* src_base, char* dst_base, float alpha, float beta,
                                          const block_side& bsa, const block_side& bsc, bool p2, float* tile,
                                          uint32_t* red) {
    using Ss = typename Es::st;
    using Sd = typename Ed::st;
    using Q = typename bq_of<Ed>::type;
    constexpr bool HAS_SA = !std::is_same<Es, f32_e>::value;
    constexpr int P = sshape<float>::P;
    constexpr int NQ = QUANT ? 2 : 1, NS = NQ * NQ;  // sub-tiles of the region
    const costa_tile_op_t& op = sop.op;
    const int rf = FULL ? NQ * SBF : rf_;
    const int rs = FULL ? NQ * SBS : rs_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const bool vd = FULL || (flags & COSTA_TILE_VEC_DST);
    const int64_t lds = op.lds, ldd = op.ldd;
    const bool frow = flags & COSTA_SCALED_F_ROWS;
    const bool tr = flags & COSTA_TILE_TRANSPOSE;
    // target coordinates of the region's origin along f and along s
    const int64_t F0 = int64_t(frow ? sop.row0 : sop.col0) + f0, S0 = int64_t(frow ? sop.col0 : sop.row0) + s0;
    const fs_side sa = along(bsa, frow), sc = along(bsc, frow);
    const Ss* src = reinterpret_cast<const Ss*>(src_base + op.src) + (int64_t(s0) * lds + f0);
    Sd* dst = reinterpret_cast<Sd*>(dst_base + op.dst) + (tr ? int64_t(f0) * ldd + s0 : int64_t(s0) * ldd + f0);
    const int t = int(threadIdx.x), lane = t % 64, wave = t / 64;
    const int lf = (t % SLPC) * SV;
    const int c0 = t / SLPC;
    // lane's strip of sub-tile q, pass k: f, s within the region and the elements it holds
    auto fq = [&](int q) { return (q % NQ) * SBF + lf; };
    auto sq = [&](int q, int k) { return (q / NQ) * SBS + c0 + k * SCPP; };
    auto held = [&](int q, int k) { return FULL || (fq(q) < rf && sq(q, k) < rs); };

    // ---- load phase: all loads issued first
    strip<Ss> x[NS][SPL];
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            x[q][k] = strip<Ss>{};
            if (held(q, k)) x[q][k] = load_strip(src + sq(q, k) * lds + fq(q), FULL ? SV : rf - fq(q), vs);
        }
    // the input scales (default cache policy); elements outside the region take 1.0
    [[maybe_unused]] float sav[NS][SPL][SV];
    if constexpr (HAS_SA) {
        const bool one = sa.f_shift == 7 && (F0 & 3) == 0;  // a strip lies inside one block
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int k = 0; k < SPL; ++k) {
#pragma unroll
                for (int e = 0; e < SV; ++e) {
                    sav[q][k][e] = 1.0f;
                    if ((FULL || (fq(q) + e < rf && sq(q, k) < rs)) && (e == 0 || !one))
                        sav[q][k][e] = sa.data[sa.at(F0 + fq(q) + e, S0 + sq(q, k))];
                }
                if (one) {
#pragma unroll
                    for (int e = 1; e < SV; ++e) sav[q][k][e] = sav[q][k][0];
                }
            }
    }
    // store unit k of this lane in transpose mode (as scaled_kernel), within sub-tile q: after the lane
    // exchange lane (base + j) stores f = u*4 + j for s = base .. base + 3
    const int j = lane & (SV - 1);
    auto unit = [&](int q, int k, int& f, int& sb, int& n_s) {
        f = (q % NQ) * SBF + (wave + SNW * k) * SV + j;
        sb = (q / NQ) * SBS + lane - j;
        n_s = FULL ? SV : rs - sb;
        return FULL || (f < rf && n_s > 0);
    };
    // dequantise with beta != 0: the old destination values, requested with the source loads
    [[maybe_unused]] strip<Sd> old[SPL];
    if constexpr (!QUANT) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            old[k] = strip<Sd>{};
            if (kind != COSTA_SCALE_AXPBY) continue;
            if (!tr) {
                if (held(0, k)) old[k] = load_strip(dst + sq(0, k) * ldd + lf, FULL ? SV : rf - lf, vd);
            } else {
                int f, sb, n_s;
                if (unit(0, k, f, sb, n_s)) old[k] = load_strip(dst + f * ldd + sb, n_s, vd);
            }
        }
    }

    // ---- x = w(a) * SA; QUANT: v = g(x) in the load arrangement
    float a[NS][SPL][SV];
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
        for (int k = 0; k < SPL; ++k)
#pragma unroll
            for (int e = 0; e < SV; ++e) {
                float v = Es::widen(x[q][k].e[e]);
                if constexpr (HAS_SA) v = v * sav[q][k][e];
                if constexpr (QUANT) v = scale<float>(v, 0.0f, kind, false, alpha, beta);
                a[q][k][e] = v;
            }

    // ---- QUANT: the block maxima (elements outside the region count as 0), S and R, the scaled data
    if constexpr (QUANT) {
        uint32_t ab[NS][SPL][SV];
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int k = 0; k < SPL; ++k)
#pragma unroll
                for (int e = 0; e < SV; ++e)
                    ab[q][k][e] = FULL || (fq(q) + e < rf && sq(q, k) < rs) ? absbits(a[q][k][e]) : 0u;
        if (sc.s_shift == 0) {
            // 128 x 1 along f: per (qs, k) one block, the DPP row's strips of both qf
#pragma unroll
            for (int qs = 0; qs < NQ; ++qs)
#pragma unroll
                for (int k = 0; k < SPL; ++k) {
                    uint32_t m = 0;
#pragma unroll
                    for (int qf = 0; qf < NQ; ++qf)
#pragma unroll
                        for (int e = 0; e < SV; ++e) m = umax(m, ab[qs * NQ + qf][k][e]);
                    m = row_max16(m);
                    const scale_pair sr = block_SR<Q>(m, p2);
                    const int s = sq(qs * NQ, k);
                    if (t % SLPC == 0 && (FULL || s < rs)) sc.data[sc.at(F0, S0 + s)] = sr.S;
#pragma unroll
                    for (int qf = 0; qf < NQ; ++qf)
#pragma unroll
                        for (int e = 0; e < SV; ++e)
                            a[qs * NQ + qf][k][e] = quant<Q>(a[qs * NQ + qf][k][e], sr.R);
                }
        } else if (sc.f_shift == 0) {
            // 1 x 128 along s: per (qf, e) one block, over both qs, the passes and all wavefronts
#pragma unroll
            for (int qf = 0; qf < NQ; ++qf)
#pragma unroll
                for (int e = 0; e < SV; ++e) {
                    uint32_t m = 0;
#pragma unroll
                    for (int qs = 0; qs < NQ; ++qs)
#pragma unroll
                        for (int k = 0; k < SPL; ++k) m = umax(m, ab[qs * NQ + qf][k][e]);
                    m = wave_rows_max(m);
                    if (lane < SLPC) red[wave * BLK + qf * SBF + lf + e] = m;
                }
            __syncthreads();
#pragma unroll
            for (int qf = 0; qf < NQ; ++qf) {
                uint32_t m[SV], w[SV];
                lds_get(m, red + qf * SBF + lf);
#pragma unroll
                for (int v = 1; v < SNW; ++v) {
                    lds_get(w, red + v * BLK + qf * SBF + lf);
#pragma unroll
                    for (int e = 0; e < SV; ++e) m[e] = umax(m[e], w[e]);
                }
#pragma unroll
                for (int e = 0; e < SV; ++e) {
                    const scale_pair sr = block_SR<Q>(m[e], p2);
                    const int f = qf * SBF + lf + e;
                    if (t < SLPC && (FULL || f < rf)) sc.data[sc.at(F0 + f, S0)] = sr.S;
#pragma unroll
                    for (int qs = 0; qs < NQ; ++qs)
#pragma unroll
                        for (int k = 0; k < SPL; ++k)
                            a[qs * NQ + qf][k][e] = quant<Q>(a[qs * NQ + qf][k][e], sr.R);
                }
            }
        } else {
            // 128 x 128: the region is one block
            uint32_t m = 0;
#pragma unroll
            for (int q = 0; q < NS; ++q)
#pragma unroll
                for (int k = 0; k < SPL; ++k)
#pragma unroll
                    for (int e = 0; e < SV; ++e) m = umax(m, ab[q][k][e]);
            m = wave_rows_max(row_max16(m));
            if (lane == 0) red[wave] = m;
            __syncthreads();
            uint32_t w[SV];
            lds_get(w, red);
            m = umax(umax(w[0], w[1]), umax(w[2], w[3]));
            const scale_pair sr = block_SR<Q>(m, p2);
            if (t == 0) sc.data[sc.at(F0, S0)] = sr.S;
#pragma unroll
            for (int q = 0; q < NS; ++q)
#pragma unroll
                for (int k = 0; k < SPL; ++k)
#pragma unroll
                    for (int e = 0; e < SV; ++e) a[q][k][e] = quant<Q>(a[q][k][e], sr.R);
        }
    }

    if (!tr) {
        // ---- copy mode: dst(f, s), no staged tile
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int k = 0; k < SPL; ++k) {
                if (!held(q, k)) continue;
                strip<Sd> o;
#pragma unroll
                for (int e = 0; e < SV; ++e) {
                    float v = a[q][k][e];
                    if constexpr (!QUANT) v = scale<float>(v, Ed::widen(old[k].e[e]), kind, false, alpha, beta);
                    o.e[e] = Ed::narrow(v);
                }
                store_strip(dst + sq(q, k) * ldd + fq(q), o, FULL ? SV : rf - fq(q), vd);
            }
        return;
    }

    // ---- transpose mode: dst(s, f) through the staged tile, one sub-tile at a time
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int qf = (q % NQ) * SBF, qs = (q / NQ) * SBS;
        if (q > 0) __syncthreads();  // (the tile's readers of sub-tile q - 1 are done)
#pragma unroll
        for (int k = 0; k < SPL; ++k)
            if (held(q, k)) lds_put(tile + (c0 + k * SCPP) * P + lf, a[q][k]);
        __syncthreads();
        float y[SPS][SV];
#pragma unroll
        for (int k = 0; k < SPS; ++k) {
            const int u = wave + SNW * k;
#pragma unroll
            for (int e = 0; e < SV; ++e) y[k][e] = 0.0f;
            if (FULL || (qs + lane < rs && qf + u * SV < rf)) lds_get(y[k], tile + lane * P + u * SV);
        }
#pragma unroll
        for (int k = 0; k < SPS; ++k) {
            transpose4(y[k], lane);  // (every lane takes part in the exchange)
            int f, sb, n_s;
            if (!unit(q, k, f, sb, n_s)) continue;
            strip<Sd> o;
#pragma unroll
            for (int e = 0; e < SV; ++e) {
                float v = y[k][e];
                if constexpr (!QUANT) v = scale<float>(v, Ed::widen(old[k].e[e]), kind, false, alpha, beta);
                o.e[e] = Ed::narrow(v);
            }
            store_strip(dst + int64_t(f) * ldd + sb, o, n_s, vd);
        }
    }
}

template <typename Es, typename Ed, bool QUANT>
__global__ __launch_bounds__(SNT) void block_kernel(const costa_scaled_op_t* __restrict__ ops,
                                                    const uint64_t* __restrict__ work, const char* src_base,
                                                    char* dst_base, const float* __restrict__ scalars,
                                                    block_side sa, block_side sc, int p2) {
    constexpr int RF = (QUANT ? 2 : 1) * SBF, RS = (QUANT ? 2 : 1) * SBS;
    uint32_t* red = nullptr;
    if constexpr (QUANT) {
        __shared__ __attribute__((aligned(16))) uint32_t blk_red[BLK_RED];
        red = blk_red;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tile = reinterpret_cast<float*>(smem);
    // which region of which op (wave-uniform: scalar loads)
    const uint64_t w = work[blockIdx.x];
    const costa_scaled_op_t sop = ops[w >> 32];
    const costa_tile_op_t& op = sop.op;
    const uint32_t sub = uint32_t(w);
    const int nbf = (op.nf + RF - 1) / RF;
    const int f0 = int(sub % uint32_t(nbf)) * RF;
    const int s0 = int(sub / uint32_t(nbf)) * RS;
    const int rf = min(RF, op.nf - f0);
    const int rs = min(RS, op.ns - s0);
    const uint32_t slot = op.flags >> COSTA_SLOT_SHIFT;
    const float alpha = scalars[2 * slot];
    const float beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (rf == RF && rs == RS && (op.flags & vec_both) == vec_both)
        run_block<Es, Ed, QUANT, true>(sop, f0, s0, rf, rs, src_base, dst_base, alpha, beta, sa, sc, p2 != 0, tile, red);
    else
        run_block<Es, Ed, QUANT, false>(sop, f0, s0, rf, rs, src_base, dst_base, alpha, beta, sa, sc, p2 != 0, tile, red);
}

template <typename Es, typename Ed, bool QUANT>
void launch_inst(const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const char* src_base,
                 char* dst_base, const void* d_scalars, const block_side& sa, const block_side& sc, bool p2,
                 hipStream_t stream) {
    launch_strip<&block_kernel<Es, Ed, QUANT>, sshape<float>::lds_bytes>(
        "block-scaled", SNT, l, stream, d_ops, d_work, src_base, dst_base, static_cast<const float*>(d_scalars), sa,
        sc, int(p2));
}

template <typename Q>
void launch_q(bool src_f, bool dst_f, const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
              const char* src_base, char* dst_base, const void* d_scalars, const block_side& sa,
              const block_side& sc, bool p2, hipStream_t s) {
    if (src_f)
        launch_inst<f32_e, q_e<Q>, true>(d_ops, d_work, l, src_base, dst_base, d_scalars, sa, sc, p2, s);
    else if (dst_f)
        launch_inst<q_e<Q>, f32_e, false>(d_ops, d_work, l, src_base, dst_base, d_scalars, sa, sc, p2, s);
    else
        launch_inst<q_e<Q>, q_e<Q>, true>(d_ops, d_work, l, src_base, dst_base, d_scalars, sa, sc, p2, s);
}

}  // namespace

bool block_pair(costa_dtype_t src, costa_dtype_t dst) {
    if (src == COSTA_FLOAT) return dtype_is_fp8(dst);
    return dtype_is_fp8(src) && (dst == COSTA_FLOAT || dst == src);
}

void block_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs) {
    if (!block_pair(src, dst))
        throw error(COSTA_ERR_ARG, std::string("costa: no block-scaled kernel for ") + dtype_name(src) + " -> " +
                                       dtype_name(dst));
    const bool quant = dtype_is_fp8(dst);
    *bf = quant ? BLK : SBF;
    *bs = quant ? BLK : SBS;
}

strip_list build_block_work(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                            const std::vector<costa_scaled_op_t>& ops, uint64_t src_base, uint64_t dst_base,
                            std::vector<costa_scaled_op_t>& ordered, std::vector<uint64_t>& work, bool dst_order) {
    const esize ES = elem_size(src_dtype), ED = elem_size(dst_dtype);
    const strip_align al = strip_alignment(strip_family::scaled, ES.qb / 4, ED.qb / 4);
    for (const costa_scaled_op_t& t : ops) {
        if (t.op.nf <= 0 || t.op.ns <= 0) continue;
        if (t.row0 < 0 || t.col0 < 0) throw error(COSTA_ERR_ARG, "costa: negative target coordinate");
    }
    return build_strip_work("block-scaled", ops, src_base, dst_base, BLK, BLK, ES, ED, al, ordered, work,
                            all_listed(), dst_order);
}

void launch_block(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* d_ops,
                  const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                  const void* d_scalars, const block_side& a_scales, const block_side& c_scales, bool pow2,
                  void* stream) {
    if (l.n_items <= 0) return;
    if (!block_pair(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, std::string("costa: no block-scaled kernel for ") + dtype_name(src_dtype) +
                                       " -> " + dtype_name(dst_dtype));
    const bool src_f = src_dtype == COSTA_FLOAT, dst_f = dst_dtype == COSTA_FLOAT;
    if ((a_scales.data != nullptr) == src_f || (c_scales.data != nullptr) == dst_f)
        throw error(COSTA_ERR_ARG, "costa: a block-scaled launch needs a scale tensor exactly on its FP8 sides");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((src_f ? dst_dtype : src_dtype) == COSTA_FP8_E4M3)
        launch_q<e4m3_t>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, a_scales, c_scales, pow2, s);
    else
        launch_q<e5m2_t>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, a_scales, c_scales, pow2, s);
}

}  // namespace engine
}  // namespace costa
