// Kernel of the dual-output MX quantise for CDNA4 (gfx950): an fp32 tile quantised twice from ONE load
// -- output 1 as mx_kernel<f32_e, Ed, QUANT> would write it, output 2 its transpose with the blocks cut
// anew (costa_hip.h, "Dual-output MX quantise").  An op is a costa_dual_op_t: the scaled op of output 1
// plus output 2's address, leading dimension and store mode.  Source element (f, s) has target
// coordinates (i, j) in output 1 and (j, i) in output 2, so output 2's fast index walks rows exactly
// where output 1's walks columns: with F0 / S0 the sub-tile's origin along f / s (the same numbers for
// both outputs) everything mx_kernels.hip says per output holds with frow2 = !frow.  Each scale tensor
// reaches the kernel in ITS output's coordinates (an mx_side); output o's blocks run along f when
// side_o.rows == frow_o.  All four combinations occur.
//
// mx_dual_kernel<Ed, SR> runs on the strip frame as mx_kernel does: 256 threads per 64 x 64 sub-tile,
// (op << 32) | sub-tile work items, source f32_e, the same lane -> strip mapping.  Phases:
//   1. load    the 4 strips of the lane, all requested first; v = g(x) once, kept unscaled in
//              registers (16 VGPRs) to the last store -- mx_kernel scales in place, this kernel cannot.
//   2. reduce  both outputs' block maxima from the same |v| bits: blocks along f through
//              half_row_max in registers (the first lane of each 8 leaves the maximum in that output's
//              `red`), blocks along s through two xor shuffles and the wavefront's partial maxima in
//              `red`.  Each output has its own 2 KiB `red`, so the two reductions need no barrier
//              between them.  If either output transposes, v is staged (unscaled) in the tile, once.
//   3. early stores  a copy-mode output whose blocks run along f has its E in registers: it is
//              quantised and stored BEFORE the barrier, so no wavefront waits before such a store.
//   4. ONE __syncthreads() for the whole sub-tile (mx_kernel: one per mode).
//   5. after it: threads 0..127 store each output's 2 x 64 scale bytes (plain stores, each byte once);
//              a copy-mode output with blocks along s reads its E from `red` and stores; the
//              transposing outputs read the staged tile ONCE (one lds_get + lane exchange per store
//              unit, shared when both transpose), take E from their `red` and store.
// A transposing output always scales after the lane exchange (mx_kernel stages scaled values when
// the blocks run along f); the products are the same single rounded multiplications, so the bytes are.
// The FULL path runs where the sub-tile is whole and the source and both destinations carry their VEC
// flags, the guarded one otherwise; elements outside tf x ts count as 0 in every maximum.  No atomics,
// no scratch.
//
// LDS words (bank = word mod 64).  `red` of an output is mx_kernel's array, written and read as
// argued in mx_kernels.hip (blocks along s: 64 consecutive words per write, conflict-free; blocks
// along f: the 8-lane write with its accepted 2-way conflict; byte stores and the per-lane E of blocks
// along s: consecutive or broadcast words).  New here: a transposing output with blocks along f reads
// red[block][sb .. sb + 3] after the barrier -- the 4 lanes of a quad share sb (broadcast), the 16
// quads of a wavefront read 64 consecutive words, and the block index (f / 32) is the same for the
// whole wavefront: conflict-free.  The two `red` arrays are 512 words apart (the same banks) but
// never touched by one instruction.  The staged tile is scaled_kernel's (rows s, pitch 68 dwords).
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "engine.hpp"
#include "mx_device.hpp"
#include "strip_device.hpp"
#include "strip_launch.hpp"
#include "strip_work.hpp"
#include "tile_device.hpp"

#pragma clang fp contract(off)

namespace costa {
namespace engine {
namespace {

// one output as the store steps see it (wave-uniform)
template <typename Sd>
struct dual_out {
    Sd* dst;           // the sub-tile's first element
    int64_t ldd;
    bool tr, vd, frow, cf;
    mx_side sc;
    uint32_t* red;
};

// the maximum of block b at line `line` of the blocks along s, after the barrier
__device__ __forceinline__ uint32_t line_max(const uint32_t* red, int b, int line) {
    uint32_t m = red[b * SBF + line];
#pragma unroll
    for (int w = 1; w < SNW; ++w) m = umax(m, red[(w * 2 + b) * SBF + line]);
    return m;
}

// phase 2 for one output: mk[k] = the maximum of the lane's block of pass k (blocks along f)
__device__ __forceinline__ void reduce_out(const uint32_t (&ab)[SPL][SV], bool cf, uint32_t* red,
                                           uint32_t (&mk)[SPL], int t, int lane, int wave, int lf, int c0) {
    if (cf) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            uint32_t m = umax(umax(ab[k][0], ab[k][1]), umax(ab[k][2], ab[k][3]));
            m = half_row_max(m);
            mk[k] = m;
            if (t % 8 == 0) red[((t % SLPC) / 8) * SBS + c0 + k * SCPP] = m;
        }
    } else {
#pragma unroll
        for (int k = 0; k < SPL; ++k) mk[k] = 0u;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < SV; ++e) {
                uint32_t m = umax(ab[2 * b][e], ab[2 * b + 1][e]);
                m = umax(m, uint32_t(__shfl_xor(m, 16)));
                m = umax(m, uint32_t(__shfl_xor(m, 32)));
                if (lane < SLPC) red[(wave * 2 + b) * SBF + lf + e] = m;
            }
    }
}

// a copy-mode output: dst(f, s) from the load arrangement.  Blocks along f: E from mk (before the
// barrier); along s: from `red` (after it)
template <typename Ed, bool SR, bool FULL>
__device__ __forceinline__ void copy_store(const float (&a)[SPL][SV], const uint32_t (&mk)[SPL],
                                           const dual_out<typename Ed::st>& o, int64_t F0, int64_t S0, int tf,
                                           int ts, bool ceil, int lf, int c0, uint32_t k0, uint32_t k1) {
    using Q = typename q_of<Ed>::type;
    const int nf_lane = FULL ? SV : tf - lf;
    uint32_t Eb[2][SV];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < SV; ++e) Eb[b][e] = o.cf ? 0u : block_E<Q>(line_max(o.red, b, lf + e), ceil);
    // SR: element (F0 + lf + e, S0 + s) of pass k; its row is F (one inner hash per e) or S (one per pass)
    [[maybe_unused]] uint32_t rh[SV];
    if constexpr (SR) {
        static_assert(SPL == SV, "one inner hash per element or per pass");
#pragma unroll
        for (int e = 0; e < SV; ++e)
            rh[e] = fmix32((o.frow ? uint32_t(F0) + uint32_t(lf + e) : uint32_t(S0) + uint32_t(c0 + e * SCPP)) ^ k0);
    }
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = c0 + k * SCPP;
        if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
        const uint32_t Ek = block_E<Q>(mk[k], ceil);
        strip<typename Ed::st> q;
#pragma unroll
        for (int e = 0; e < SV; ++e) {
            const float v = quant<Q>(a[k][e], o.cf ? Ek : Eb[k / 2][e]);
            if constexpr (SR)
                q.e[e] = Ed::narrow_sr(v, o.frow ? sr_bits(rh[e], uint32_t(S0) + uint32_t(s), k1)
                                                 : sr_bits(rh[k], uint32_t(F0) + uint32_t(lf + e), k1));
            else
                q.e[e] = Ed::narrow(v);
        }
        store_at<Ed>(o.dst, s * o.ldd + lf, q, nf_lane, o.vd);
    }
}

// a transposing output: dst(s, f) from the exchanged strips y (lane (base + j) holds f = q*4 + j for
// s = base .. base + 3), E from `red` after the barrier
template <typename Ed, bool SR, bool FULL>
__device__ __forceinline__ void tr_store(const float (&y)[SPS][SV], const dual_out<typename Ed::st>& o, int64_t F0,
                                         int64_t S0, int tf, int ts, bool ceil, int lane, int wave, uint32_t k0,
                                         uint32_t k1) {
    using Q = typename q_of<Ed>::type;
    const int j = lane & (SV - 1), sb = lane - j;
    const int n_s = FULL ? SV : ts - sb;
    [[maybe_unused]] uint32_t rh[SV];
    if constexpr (SR) {
        static_assert(SPS == SV, "one inner hash per unit or per element");
#pragma unroll
        for (int e = 0; e < SV; ++e)
            rh[e] = fmix32((o.frow ? uint32_t(F0) + uint32_t((wave + SNW * e) * SV + j)
                                   : uint32_t(S0) + uint32_t(sb + e)) ^ k0);
    }
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        const int f = (wave + SNW * k) * SV + j;
        if (!FULL && (f >= tf || n_s <= 0)) continue;
        // blocks along s: a strip along s lies in one block; along f: one block per element
        const uint32_t Es = o.cf ? 0u : block_E<Q>(line_max(o.red, sb / MXB, f), ceil);
        strip<typename Ed::st> q;
#pragma unroll
        for (int e = 0; e < SV; ++e) {
            const uint32_t E = o.cf ? block_E<Q>(o.red[(f / MXB) * SBS + sb + e], ceil) : Es;
            const float v = quant<Q>(y[k][e], E);
            if constexpr (SR)
                q.e[e] = Ed::narrow_sr(v, o.frow ? sr_bits(rh[k], uint32_t(S0) + uint32_t(sb + e), k1)
                                                 : sr_bits(rh[e], uint32_t(F0) + uint32_t(f), k1));
            else
                q.e[e] = Ed::narrow(v);
        }
        store_at<Ed>(o.dst, f * o.ldd + sb, q, n_s, o.vd);
    }
}

// after the barrier: threads 0..127 store the output's 2 x 64 scale bytes
template <typename Ed, bool FULL>
__device__ __forceinline__ void store_bytes(const dual_out<typename Ed::st>& o, int64_t F0, int64_t S0, int tf,
                                            int ts, bool ceil, int t) {
    using Q = typename q_of<Ed>::type;
    if (t >= 2 * 64) return;
    const int b = t / 64, line = t % 64;
    const uint32_t m = o.cf ? o.red[b * SBS + line] : line_max(o.red, b, line);
    const int n_axis = o.cf ? tf : ts, n_line = o.cf ? ts : tf;
    if (!FULL && (b * MXB >= n_axis || line >= n_line)) return;
    const int64_t B = (o.cf ? F0 : S0) / MXB + b, L = (o.cf ? S0 : F0) + line;
    static_cast<uint8_t*>(o.sc.data)[B * o.sc.block_stride + L * o.sc.line_stride] = uint8_t(block_E<Q>(m, ceil));
}

template <typename Ed, bool SR, bool FULL>
__device__ __forceinline__ void run_dual(const costa_dual_op_t& dop, int f0, int s0, int tf_, int ts_,
                                         const char* src_base, char* dst_base, char* dst2_base, float alpha,
                                         float beta, const mx_side& sc1, const mx_side& sc2, bool ceil, float* tile,
                                         uint32_t* red1, uint32_t* red2, uint32_t k0, uint32_t k1) {
    using Sd = typename Ed::st;
    constexpr int P = sshape<float>::P;
    const costa_tile_op_t& op = dop.s.op;
    const int tf = FULL ? SBF : tf_;
    const int ts = FULL ? SBS : ts_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const int64_t lds = op.lds;
    const bool frow = flags & COSTA_SCALED_F_ROWS;
    // the sub-tile's origin along f and along s: output 1's target coordinates, and output 2's with
    // rows and columns swapped and frow complemented -- the same two numbers
    const int64_t F0 = int64_t(frow ? dop.s.row0 : dop.s.col0) + f0, S0 = int64_t(frow ? dop.s.col0 : dop.s.row0) + s0;
    const float* src = reinterpret_cast<const float*>(src_base + op.src) + (int64_t(s0) * lds + f0);
    const int t = int(threadIdx.x), lane = t % 64, wave = t / 64;

    dual_out<Sd> o1, o2;
    o1.tr = flags & COSTA_TILE_TRANSPOSE;
    o1.vd = FULL || (flags & COSTA_TILE_VEC_DST);
    o1.frow = frow;
    o1.cf = sc1.rows == frow;
    o1.sc = sc1;
    o1.red = red1;
    o1.ldd = op.ldd;
    o1.dst = reinterpret_cast<Sd*>(dst_base + op.dst) +
             elems<Ed>(o1.tr ? int64_t(f0) * o1.ldd + s0 : int64_t(s0) * o1.ldd + f0);
    o2.tr = dop.flags2 & COSTA_TILE_TRANSPOSE;
    o2.vd = FULL || (dop.flags2 & COSTA_TILE_VEC_DST);
    o2.frow = !frow;
    o2.cf = sc2.rows == !frow;
    o2.sc = sc2;
    o2.red = red2;
    o2.ldd = dop.ldd2;
    o2.dst = reinterpret_cast<Sd*>(dst2_base + dop.dst2) +
             elems<Ed>(o2.tr ? int64_t(f0) * o2.ldd + s0 : int64_t(s0) * o2.ldd + f0);

    // ---- 1. load phase: lane -> (strip along f, column s); all loads issued first
    const int lf = (t % SLPC) * SV;
    const int c0 = t / SLPC;
    const int nf_lane = FULL ? SV : tf - lf;
    strip<float> x[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = c0 + k * SCPP;
        x[k] = strip<float>{};
        if (FULL || (nf_lane > 0 && s < ts)) x[k] = load_at<f32_e>(src, s * lds + lf, nf_lane, vs);
    }
    float a[SPL][SV];
    uint32_t ab[SPL][SV];
#pragma unroll
    for (int k = 0; k < SPL; ++k)
#pragma unroll
        for (int e = 0; e < SV; ++e) {
            a[k][e] = scale<float>(x[k].e[e], 0.0f, kind, false, alpha, beta);
            ab[k][e] = FULL || (lf + e < tf && c0 + k * SCPP < ts) ? absbits(a[k][e]) : 0u;
        }

    // ---- 2. both reductions; the staged tile where an output transposes
    uint32_t mk1[SPL], mk2[SPL];
    reduce_out(ab, o1.cf, red1, mk1, t, lane, wave, lf, c0);
    reduce_out(ab, o2.cf, red2, mk2, t, lane, wave, lf, c0);
    const bool any_tr = o1.tr || o2.tr;
    if (any_tr) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int s = c0 + k * SCPP;
            if (FULL || (nf_lane > 0 && s < ts)) lds_put(tile + s * P + lf, a[k]);
        }
    }
    // ---- 3. copy-mode outputs with their E in registers: stored before the barrier
    if (!o1.tr && o1.cf) copy_store<Ed, SR, FULL>(a, mk1, o1, F0, S0, tf, ts, ceil, lf, c0, k0, k1);
    if (!o2.tr && o2.cf) copy_store<Ed, SR, FULL>(a, mk2, o2, F0, S0, tf, ts, ceil, lf, c0, k0, k1);
    // ---- 4. the sub-tile's one barrier
    __syncthreads();
    // ---- 5. scale bytes, then the outputs that need `red` or the staged tile
    store_bytes<Ed, FULL>(o1, F0, S0, tf, ts, ceil, t);
    store_bytes<Ed, FULL>(o2, F0, S0, tf, ts, ceil, t);
    if (!o1.tr && !o1.cf) copy_store<Ed, SR, FULL>(a, mk1, o1, F0, S0, tf, ts, ceil, lf, c0, k0, k1);
    if (!o2.tr && !o2.cf) copy_store<Ed, SR, FULL>(a, mk2, o2, F0, S0, tf, ts, ceil, lf, c0, k0, k1);
    if (!any_tr) return;
    float y[SPS][SV];
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        const int q = wave + SNW * k;
#pragma unroll
        for (int e = 0; e < SV; ++e) y[k][e] = 0.0f;
        if (FULL || (lane < ts && q * SV < tf)) lds_get(y[k], tile + lane * P + q * SV);
        transpose4(y[k], lane);  // (every lane takes part in the exchange)
    }
    if (o1.tr) tr_store<Ed, SR, FULL>(y, o1, F0, S0, tf, ts, ceil, lane, wave, k0, k1);
    if (o2.tr) tr_store<Ed, SR, FULL>(y, o2, F0, S0, tf, ts, ceil, lane, wave, k0, k1);
}

// SR instances take the two 32-bit keys of the call's seed behind `ceil`; the others no argument more
template <typename Ed, bool SR, typename... Keys>
__global__ __launch_bounds__(SNT) void mx_dual_kernel(const costa_dual_op_t* __restrict__ ops,
                                                      const uint64_t* __restrict__ work, const char* src_base,
                                                      char* dst_base, char* dst2_base,
                                                      const float* __restrict__ scalars, mx_side sc1, mx_side sc2,
                                                      int ceil, Keys... keys) {
    static_assert(sizeof...(Keys) == (SR ? 2 : 0), "k0, k1 with SR only");
    uint32_t k0 = 0, k1 = 0;
    if constexpr (SR) {
        const uint32_t kk[2] = {keys...};
        k0 = kk[0];
        k1 = kk[1];
    }
    __shared__ uint32_t mx_red[2][MX_RED];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tile = reinterpret_cast<float*>(smem);
    // which sub-tile of which op (wave-uniform: scalar loads)
    const uint64_t w = work[blockIdx.x];
    const costa_dual_op_t dop = ops[w >> 32];
    const costa_tile_op_t& op = dop.s.op;
    const uint32_t sub = uint32_t(w);
    const int nbf = (op.nf + SBF - 1) / SBF;
    const int f0 = int(sub % uint32_t(nbf)) * SBF;
    const int s0 = int(sub / uint32_t(nbf)) * SBS;
    const int tf = min(SBF, op.nf - f0);
    const int ts = min(SBS, op.ns - s0);
    const uint32_t slot = op.flags >> COSTA_SLOT_SHIFT;
    const float alpha = scalars[2 * slot];
    const float beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (tf == SBF && ts == SBS && (op.flags & vec_both) == vec_both && (dop.flags2 & COSTA_TILE_VEC_DST))
        run_dual<Ed, SR, true>(dop, f0, s0, tf, ts, src_base, dst_base, dst2_base, alpha, beta, sc1, sc2, ceil != 0,
                               tile, mx_red[0], mx_red[1], k0, k1);
    else
        run_dual<Ed, SR, false>(dop, f0, s0, tf, ts, src_base, dst_base, dst2_base, alpha, beta, sc1, sc2, ceil != 0,
                                tile, mx_red[0], mx_red[1], k0, k1);
}

template <typename EQ>  // the codec of the outputs' type: q_e<Q>, q4_e or q6_e<T>
void launch_q(const costa_dual_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const char* src_base,
              char* dst_base, char* dst2_base, const void* d_scalars, const mx_side& sc1, const mx_side& sc2,
              bool ceil, const mx_sr* sr, hipStream_t s) {
    if (sr)
        launch_strip<&mx_dual_kernel<EQ, true, uint32_t, uint32_t>, sshape<float>::lds_bytes>(
            "MX dual", SNT, l, s, d_ops, d_work, src_base, dst_base, dst2_base, static_cast<const float*>(d_scalars),
            sc1, sc2, int(ceil), sr->k0, sr->k1);
    else
        launch_strip<&mx_dual_kernel<EQ, false>, sshape<float>::lds_bytes>(
            "MX dual", SNT, l, s, d_ops, d_work, src_base, dst_base, dst2_base, static_cast<const float*>(d_scalars),
            sc1, sc2, int(ceil));
}

}  // namespace

strip_list build_dual_work(costa_dtype_t dst_dtype, const std::vector<costa_dual_op_t>& ops, uint64_t src_base,
                           uint64_t dst_base, uint64_t dst2_base, std::vector<costa_dual_op_t>& ordered,
                           std::vector<uint64_t>& work, bool dst_order) {
    const esize ES = elem_size(COSTA_FLOAT), ED = elem_size(dst_dtype);
    strip_align al = strip_alignment(strip_family::scaled, 4, std::max<uint64_t>(1, ED.qb / 4));
    if (dtype_is_fp4(dst_dtype)) al.dst = 2;
    if (dtype_is_fp6(dst_dtype)) al.dst = 1;
    for (const costa_dual_op_t& t : ops) {  // (empty ops are skipped unchecked, as by the builder)
        if (t.s.op.nf <= 0 || t.s.op.ns <= 0) continue;
        if (t.s.op.lds < 0 || t.s.op.ldd < 0 || t.ldd2 < 0) throw error(COSTA_ERR_ARG, "costa: negative leading dimension");
        if (t.s.row0 < 0 || t.s.col0 < 0) throw error(COSTA_ERR_ARG, "costa: negative target coordinate");
    }
    strip_list l = build_strip_work("dual", ops, src_base, dst_base, SBF, SBS, ES, ED, al, ordered, work, all_listed(),
                                    dst_order);
    // output 2's side: its VEC flag by the same rule at its own address, and its store mode
    for (costa_dual_op_t& t : ordered) {
        t.flags2 &= COSTA_TILE_TRANSPOSE;
        if ((dst2_base + t.dst2) % al.dst == 0 && ED.bytes(uint64_t(t.ldd2)) % al.dst == 0)
            t.flags2 |= COSTA_TILE_VEC_DST;
        if (t.flags2 & COSTA_TILE_TRANSPOSE) l.any_transpose = true;
    }
    return l;
}

void launch_mx_dual(costa_dtype_t dst_dtype, const costa_dual_op_t* d_ops, const uint64_t* d_work,
                    const strip_list& l, const char* src_base, char* dst_base, char* dst2_base,
                    const void* d_scalars, const mx_side& c_scales, const mx_side& ct_scales, bool ceil,
                    void* stream, const mx_sr* sr) {
    if (l.n_items <= 0) return;
    if (!mx_pair(COSTA_FLOAT, dst_dtype) || dst_dtype == COSTA_FLOAT)
        throw error(COSTA_ERR_ARG, std::string("costa: no dual MX kernel for FLOAT -> ") + dtype_name(dst_dtype));
    if (!c_scales.data || !ct_scales.data)
        throw error(COSTA_ERR_ARG, "costa: a dual MX launch needs both scale tensors");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dst_dtype == COSTA_FP8_E4M3)
        launch_q<q_e<e4m3_t>>(d_ops, d_work, l, src_base, dst_base, dst2_base, d_scalars, c_scales, ct_scales, ceil, sr, s);
    else if (dst_dtype == COSTA_FP8_E5M2)
        launch_q<q_e<e5m2_t>>(d_ops, d_work, l, src_base, dst_base, dst2_base, d_scalars, c_scales, ct_scales, ceil, sr, s);
    else if (dst_dtype == COSTA_FP4_E2M1)
        launch_q<q4_e>(d_ops, d_work, l, src_base, dst_base, dst2_base, d_scalars, c_scales, ct_scales, ceil, sr, s);
    else if (dst_dtype == COSTA_FP6_E2M3)
        launch_q<q6_e<e2m3_t>>(d_ops, d_work, l, src_base, dst_base, dst2_base, d_scalars, c_scales, ct_scales, ceil, sr, s);
    else
        launch_q<q6_e<e3m2_t>>(d_ops, d_work, l, src_base, dst_base, dst2_base, d_scalars, c_scales, ct_scales, ceil, sr, s);
}

}  // namespace engine
}  // namespace costa
