// Kernels of MX block-scaled transforms for CDNA4 (gfx950): tile ops whose FP8 side carries one E8M0
// scale byte per 32 consecutive elements along one axis (costa_hip.h, "MX block-scaled transforms").
// An op is a costa_scaled_op_t, as for scaled_kernel: with COSTA_SCALED_F_ROWS the op's fast index f
// walks target rows (i = row0 + f, j = col0 + s), else columns.  Both scale tensors reach the kernel
// in TARGET coordinates (an mx_side: the host has already turned A's axis round for a transposing
// job), so a block runs along f when `side.rows == F_ROWS` and along s otherwise.  With pow2(E) the
// fp32 of a scale byte, w() / cvt() the codecs of tile_device.hpp and g() tile_kernel's scale<float>
// (contraction off), an op computes per element
//   x = w(a) [* pow2(SA[block of a])]            one rounded product
//   v = g(x, w(c_old))
//   dequantise (no c_scales): store v
//   quantise / requantise: per block of C, amax = unsigned max of the bits of |v|, e = amax >> 23,
//     E = 255 and NaN everywhere when e == 255, else E = max(e - emax, 0) (CEIL: one more when
//     amax * pow2(254 - E) > fmax), q = cvt(clamp(v * pow2(254 - E), -fmax, fmax)), SC[block] = E.
//
// One family, mx_kernel<Es, Ed, QUANT, SR>, on the strip frame (strip_device.hpp, strip_work.hpp,
// strip_launch.hpp): 256 threads per 64 x 64 sub-tile, (op << 32) | sub-tile work items.  The planner
// and costa_hip_execute_tiles_mx guarantee that an op starts on a multiple of 32 of C's block axis,
// and 64 is a multiple of 32, so a sub-tile holds 2 x 64 whole blocks (the last may be partial at the
// matrix edge), every block belongs to one workgroup and every scale byte is written once, by a
// plain vector store: no atomics.
//
// Load phase (both modes, as scaled_kernel): lane t holds strips x[k] at f = (t % 16) * 4 + e,
// s = t / 16 + 16 k.  The source strips, the old destination strips (dequantise, beta != 0) and
// the input scale bytes are all requested before the first use.  Input scale bytes use the default
// cache policy (the neighbouring sub-tiles of the block row / column read them again), data the
// non-temporal accesses of the strip loads and stores.  Where SA's blocks run along f and the
// sub-tile's origin along f is a multiple of 4 in target coordinates, a strip lies inside one block
// and takes one byte load; otherwise each element indexes its own byte (same values).
// With beta = 0 (required with c_scales) v depends on x alone, so QUANT instantiations compute v in
// the load arrangement and reduce there, the same in copy and transpose mode:
//   blocks along f   a block is the strips of 8 consecutive lanes (half a DPP row) at one s: the
//                    maximum of a strip's 4 elements, then quad_perm [1,0,3,2], quad_perm [2,3,0,1]
//                    and row_half_mirror give every lane its block's maximum: E in registers, no
//                    barrier before the data is scaled.  The first lane of the 8 leaves the maximum
//                    in LDS (red[block][s], 128 words) for the byte stores.
//   blocks along s   block 0 is passes k = 0, 1 and block 1 passes k = 2, 3 of all 4 wavefronts: the
//                    maximum over a block's two passes per element, two xor shuffles (16, 32) over
//                    the wavefront's 4 rows, then the wavefront's 2 x 64 partial maxima go to LDS
//                    (red[wave][block][f], 512 words = 2 KiB) and meet after the mode's ONE barrier:
//                    in transpose mode the staged tile's own (v is staged unscaled and each lane
//                    scales its strip along s, which lies in one block, after the lane exchange); in
//                    copy mode a barrier before the stores.
// After the barrier threads 0..127 store the 2 x 64 scale bytes (thread -> block t / 64, line
// t % 64): with line_stride = 1 a wavefront writes 64 consecutive bytes, with block_stride = 1 the
// two blocks of a line are neighbours.  Blocks-along-f copy mode puts the barrier after the data
// stores, so no wavefront waits before it stores.
// LDS words of `red` (bank = word mod 64).  Writes, blocks along s: the wavefront's first 16 lanes
// write 4 consecutive words each, 64 consecutive words per (block, element pass): conflict-free.
// Writes, blocks along f: 8 lanes of a wavefront write red[block][s] for 4 consecutive s and both
// blocks; the two blocks of one s lie 64 words apart and share a bank: 2-way on an 8-lane write, 4
// such writes per sub-tile (accepted).  Reads after the barrier: the byte stores read consecutive
// words per wavefront; the per-lane E of blocks along s reads, in copy mode, 4 consecutive words per
// lane with the 16 lanes of a row on 64 consecutive words and the wavefront's 4 rows on the same
// words (broadcast), and in transpose mode the same 4 consecutive words in every quad (broadcast).
// The staged tile is scaled_kernel's: rows s, pitch 68 dwords, conflict-free as argued there.
// Whole sub-tiles with both VEC flags take the FULL path; remainders and unaligned sides the guarded
// one, where elements outside tf x ts count as 0 in every maximum whatever alpha is.  No scratch.
//
// Packed e2m1 (COSTA_FP4_E2M1; costa_hip.h, "MXFP4"): the codec q4_e beside q_e<Q>, three more
// instantiations (f32_e -> q4_e QUANT, q4_e -> f32_e, q4_e -> q4_e QUANT) of the same kernel: the load
// arrangement, both block reductions, the single barrier per mode, the 2 x 64 scale-byte stores and
// the FULL / guarded split are shared line for line.  A strip of 4 elements is 2 bytes along the
// side's stored-contiguous dimension -- f for the source, f for a copy-mode destination, s for a
// transpose-mode one: the directions the strips already run in -- and holds its 4 codes unpacked, one
// per byte of strip<uint8_t>, between load_strip4 and store_strip4.  Every element offset the kernel
// forms on an FP4 side is even (the evenness rule: even ld, even extents; f0, s0, lf and sb are
// multiples of 4), so elems() halves it exactly.  With the side's VEC flag (first byte at an even
// address, ld a multiple of 4) a whole strip is one 2-byte access; otherwise one or two byte accesses
// (ld = 2 mod 4 puts every other line on an odd byte).  A partial strip holds 2 elements: one whole
// byte.  A destination byte is always written whole, by one lane: no read-modify-write, no atomics.
// cvt4 is the FP8 codec's round_finite with one mantissa bit and bias 1 (integer rounding to nearest
// even on the dropped bits, which is the type's tie rule; below 1.0 one exact fp32 addition; the sign
// bit kept, NaN -> 0x0), w4 a shift and two selects; the gfx950 packed FP4 conversion instructions are
// not used.  LDS: the codec adds and changes no LDS access -- the staged
// tile holds fp32 v and `red` fp32 bit patterns exactly as for FP8, so the bank behaviour above
// stands unchanged.
//
// Packed FP6 (COSTA_FP6_E2M3 / COSTA_FP6_E3M2; costa_hip.h, "MXFP6"): the codecs q6_e<e2m3_t> /
// q6_e<e3m2_t> and six more instantiations (f32_e -> q6_e QUANT, q6_e -> f32_e, q6_e -> q6_e QUANT per
// type) of the same kernel; everything named above as shared stays shared line for line.  A strip of 4
// elements is exactly one packing group: 3 bytes along the side's stored-contiguous dimension, its 4
// codes unpacked one per byte of strip<uint8_t> between load_strip6 and store_strip6.  Every element
// offset the kernel forms on an FP6 side is a multiple of 4 (the quad rule: ld and extents are
// multiples of 4; f0, s0, lf and sb are multiples of 4), so elems() = (at >> 2) * 3 is exact, a strip
// starts on a group boundary, and a group never straddles two lanes: strips are 4 elements, groups
// are 4 elements, and both count from the op's first element.  For the same reason a strip on an FP6
// side is whole or absent (tf / ts are multiples of 4 along that side's contiguous direction): there
// are no partial groups.  Access widths on an FP6 side: two non-temporal accesses per strip, 2 bytes
// at p and 1 byte at p + 2.  Byte addresses have any parity (an op may start on an odd byte, and
// ld = 4 mod 8 gives an odd byte pitch, so consecutive lines alternate parity); the 2-byte access is
// made through a type of alignment 1 -- global memory takes it at an odd address, and written as two
// byte accesses the compiler merges them into the same instruction anyway, but drops the load's
// non-temporal hint -- so nothing is asked of the address, the side's VEC flag is vacuous
// (strip_work.hpp gives it alignment 1) and the FULL / guarded split follows the other side's flag
// and the sub-tile's extents alone.  No access,
// reads included, touches a byte outside the 3 bytes of its own group, so the last group of a tile
// may be the last three bytes of an allocation; a destination group is written whole by one lane: no
// read-modify-write, no atomics.  cvt6 is round_finite<3, 1> / round_finite<2, 3> with the sign bit
// kept and NaN -> 0x00, w6 a shift and a select (subnormal codes: an exact int -> fp32 conversion
// times the step); the gfx950 packed FP6 conversion instructions are not used.  LDS: as for FP4, the
// staged tile holds fp32 v and `red` fp32 bit patterns, so the bank argument above stands unchanged.
//
// Stochastic rounding (costa_hip.h, "Stochastic rounding in the MX transforms"): the template flag SR,
// valid with QUANT, gives ten more instantiations (f32_e -> Q, Q -> Q for the five codecs) that differ
// from the plain ones at the two store sites alone: Ed::narrow_sr(v, U) in place of Ed::narrow(v), U
// the 24 hashed bits of the element's row and column in C's matrix under the call's two 32-bit keys
// (kernel arguments of the SR instantiations only).  The target coordinates are in registers at both
// sites -- copy mode (F0 + lf + e, S0 + s), transpose mode after the lane exchange (F0 + f,
// S0 + sb + e), (i, j) through F_ROWS -- and a lane's 16 elements lie in 4 rows of C either way, so
// the row's inner fmix32 runs 4 times per lane and the outer one once per element.  Integer VALU code;
// no LDS access, no barrier and no memory access is added or moved.  No scratch.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "engine.hpp"
#include "mx_device.hpp"
#include "strip_device.hpp"
#include "strip_launch.hpp"
#include "tile_device.hpp"

#pragma clang fp contract(off)

namespace costa {
namespace engine {
namespace {

// (qlim, block_E, quant, pow2, half_row_max, fmix32, sr_bits, elems / load_at / store_at: mx_device.hpp,
// shared with mx_dual_kernels.hip)

template <typename Es, typename Ed, bool QUANT, bool SR, bool FULL>
__device__ __forceinline__ void run_mx(const costa_scaled_op_t& sop, int f0, int s0, int tf_, int ts_,
                                       const char* src_base, char* dst_base, float alpha, float beta,
                                       const mx_side& sa, const mx_side& sc, bool ceil, float* tile,
                                       uint32_t* red, uint32_t k0, uint32_t k1) {
    static_assert(QUANT || !SR, "stochastic rounding belongs to the quantising instances");
    using Ss = typename Es::st;
    using Sd = typename Ed::st;
    using Q = typename q_of<Ed>::type;
    constexpr bool HAS_SA = !std::is_same<Es, f32_e>::value;
    constexpr int P = sshape<float>::P;
    const costa_tile_op_t& op = sop.op;
    const int tf = FULL ? SBF : tf_;
    const int ts = FULL ? SBS : ts_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const bool vd = FULL || (flags & COSTA_TILE_VEC_DST);
    const int64_t lds = op.lds, ldd = op.ldd;
    const bool frow = flags & COSTA_SCALED_F_ROWS;
    // target coordinates of the sub-tile's origin along f and along s
    const int64_t F0 = int64_t(frow ? sop.row0 : sop.col0) + f0, S0 = int64_t(frow ? sop.col0 : sop.row0) + s0;
    const bool sa_f = sa.rows == frow;  // A's blocks run along f
    const bool cf = sc.rows == frow;    // C's blocks run along f (QUANT)
    const Ss* src = reinterpret_cast<const Ss*>(src_base + op.src) + elems<Es>(int64_t(s0) * lds + f0);
    const int t = int(threadIdx.x), lane = t % 64, wave = t / 64;

    // ---- load phase: lane -> (strip along f, column s); all loads issued first
    const int lf = (t % SLPC) * SV;
    const int c0 = t / SLPC;
    const int nf_lane = FULL ? SV : tf - lf;
    strip<Ss> x[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = c0 + k * SCPP;
        x[k] = strip<Ss>{};
        if (FULL || (nf_lane > 0 && s < ts)) x[k] = load_at<Es>(src, s * lds + lf, nf_lane, vs);
    }
    // the input scale bytes (default cache policy); elements outside the sub-tile take 127 (1.0)
    [[maybe_unused]] uint32_t sab[SPL][SV];
    if constexpr (HAS_SA) {
        const uint8_t* sp = static_cast<const uint8_t*>(sa.data);
        const bool one = sa_f && (F0 & 3) == 0;  // a strip lies inside one block
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int s = c0 + k * SCPP;
#pragma unroll
            for (int e = 0; e < SV; ++e) {
                sab[k][e] = 127u;
                if ((FULL || (lf + e < tf && s < ts)) && (e == 0 || !one)) {
                    const int64_t F = F0 + lf + e, S = S0 + s;
                    const int64_t at = sa_f ? (F / MXB) * sa.block_stride + S * sa.line_stride
                                            : (S / MXB) * sa.block_stride + F * sa.line_stride;
                    sab[k][e] = sp[at];
                }
            }
            if (one) {
#pragma unroll
                for (int e = 1; e < SV; ++e) sab[k][e] = sab[k][0];
            }
        }
    }
    const bool tr = flags & COSTA_TILE_TRANSPOSE;
    Sd* dst = reinterpret_cast<Sd*>(dst_base + op.dst) +
              elems<Ed>(tr ? int64_t(f0) * ldd + s0 : int64_t(s0) * ldd + f0);
    // store unit k of this lane in transpose mode (as scaled_kernel): after the lane exchange lane
    // (base + j) stores f = q*4 + j for s = base .. base + 3
    const int j = lane & (SV - 1);
    auto unit = [&](int k, int& f, int& sb, int& n_s) {
        f = (wave + SNW * k) * SV + j;
        sb = lane - j;
        n_s = FULL ? SV : ts - sb;
        return FULL || (f < tf && n_s > 0);
    };
    // dequantise with beta != 0: the old destination values, requested with the source loads
    [[maybe_unused]] strip<Sd> old[SPL];
    if constexpr (!QUANT) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            old[k] = strip<Sd>{};
            if (kind != COSTA_SCALE_AXPBY) continue;
            if (!tr) {
                const int s = c0 + k * SCPP;
                if (FULL || (nf_lane > 0 && s < ts)) old[k] = load_strip(dst + s * ldd + lf, nf_lane, vd);
            } else {
                int f, sb, n_s;
                if (unit(k, f, sb, n_s)) old[k] = load_strip(dst + f * ldd + sb, n_s, vd);
            }
        }
    }

    // ---- x = w(a) * pow2(SA); QUANT: v = g(x) in the load arrangement
    float a[SPL][SV];
#pragma unroll
    for (int k = 0; k < SPL; ++k)
#pragma unroll
        for (int e = 0; e < SV; ++e) {
            float v = Es::widen(x[k].e[e]);
            if constexpr (HAS_SA) v = v * pow2(sab[k][e]);
            if constexpr (QUANT) v = scale<float>(v, 0.0f, kind, false, alpha, beta);
            a[k][e] = v;
        }

    // ---- QUANT: the block maxima (elements outside tf x ts count as 0)
    [[maybe_unused]] uint32_t Ek[SPL];  // blocks along f: the E of the lane's block per pass
    if constexpr (QUANT) {
        uint32_t ab[SPL][SV];
#pragma unroll
        for (int k = 0; k < SPL; ++k)
#pragma unroll
            for (int e = 0; e < SV; ++e)
                ab[k][e] = FULL || (lf + e < tf && c0 + k * SCPP < ts) ? absbits(a[k][e]) : 0u;
        if (cf) {
#pragma unroll
            for (int k = 0; k < SPL; ++k) {
                uint32_t m = umax(umax(ab[k][0], ab[k][1]), umax(ab[k][2], ab[k][3]));
                m = half_row_max(m);
                Ek[k] = block_E<Q>(m, ceil);
                if (t % 8 == 0) red[((t % SLPC) / 8) * SBS + c0 + k * SCPP] = m;
#pragma unroll
                for (int e = 0; e < SV; ++e) a[k][e] = quant<Q>(a[k][e], Ek[k]);
            }
        } else {
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
    // the maximum of block b at line `line` of the blocks along s, after the barrier
    auto line_max = [&](int b, int line) {
        uint32_t m = red[b * SBF + line];
#pragma unroll
        for (int w = 1; w < SNW; ++w) m = umax(m, red[(w * 2 + b) * SBF + line]);
        return m;
    };
    // after the barrier: threads 0..127 store the sub-tile's 2 x 64 scale bytes
    auto store_bytes = [&]() {
        if constexpr (QUANT) {
            if (t >= 2 * 64) return;
            const int b = t / 64, line = t % 64;
            const uint32_t m = cf ? red[b * SBS + line] : line_max(b, line);
            const int n_axis = cf ? tf : ts, n_line = cf ? ts : tf;
            if (!FULL && (b * MXB >= n_axis || line >= n_line)) return;
            const int64_t B = (cf ? F0 : S0) / MXB + b, L = (cf ? S0 : F0) + line;
            static_cast<uint8_t*>(sc.data)[B * sc.block_stride + L * sc.line_stride] = uint8_t(block_E<Q>(m, ceil));
        }
    };

    if (!tr) {
        // ---- copy mode: dst(f, s), no staged tile
        [[maybe_unused]] uint32_t Eb[2][SV];
        if constexpr (QUANT) {
            if (!cf) {
                __syncthreads();
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int e = 0; e < SV; ++e) Eb[b][e] = block_E<Q>(line_max(b, lf + e), ceil);
            }
        }
        // SR: element (F0 + lf + e, S0 + s) of pass k; its row is F (one inner hash per e, shared by the
        // passes) or S (one per pass, shared by the strip)
        [[maybe_unused]] uint32_t rh[SV];
        if constexpr (SR) {
            static_assert(SPL == SV, "one inner hash per element or per pass");
#pragma unroll
            for (int e = 0; e < SV; ++e)
                rh[e] = fmix32((frow ? uint32_t(F0) + uint32_t(lf + e) : uint32_t(S0) + uint32_t(c0 + e * SCPP)) ^ k0);
        }
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int s = c0 + k * SCPP;
            if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
            strip<Sd> o;
#pragma unroll
            for (int e = 0; e < SV; ++e) {
                float v = a[k][e];
                if constexpr (QUANT) {
                    if (!cf) v = quant<Q>(v, Eb[k / 2][e]);
                } else {
                    v = scale<float>(v, Ed::widen(old[k].e[e]), kind, false, alpha, beta);
                }
                if constexpr (SR)
                    o.e[e] = Ed::narrow_sr(v, frow ? sr_bits(rh[e], uint32_t(S0) + uint32_t(s), k1)
                                                   : sr_bits(rh[k], uint32_t(F0) + uint32_t(lf + e), k1));
                else
                    o.e[e] = Ed::narrow(v);
            }
            store_at<Ed>(dst, s * ldd + lf, o, nf_lane, vd);
        }
        if constexpr (QUANT) {
            if (cf) __syncthreads();  // (after the stores: no wavefront waits before it stores)
            store_bytes();
        }
        return;
    }

    // ---- transpose mode: dst(s, f) through the staged tile
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = c0 + k * SCPP;
        if (FULL || (nf_lane > 0 && s < ts)) lds_put(tile + s * P + lf, a[k]);
    }
    __syncthreads();
    store_bytes();
    // SR: element (F0 + f, S0 + sb + e) of unit k, sb = lane - j for every unit; its row is F (one inner
    // hash per unit, shared by the strip) or S (one per e, shared by the units)
    [[maybe_unused]] uint32_t rh[SV];
    if constexpr (SR) {
        static_assert(SPS == SV, "one inner hash per unit or per element");
#pragma unroll
        for (int e = 0; e < SV; ++e)
            rh[e] = fmix32((frow ? uint32_t(F0) + uint32_t((wave + SNW * e) * SV + j)
                                 : uint32_t(S0) + uint32_t(lane - j + e)) ^ k0);
    }
    float y[SPS][SV];
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        const int q = wave + SNW * k;
#pragma unroll
        for (int e = 0; e < SV; ++e) y[k][e] = 0.0f;
        if (FULL || (lane < ts && q * SV < tf)) lds_get(y[k], tile + lane * P + q * SV);
    }
#pragma unroll
    for (int k = 0; k < SPS; ++k) {
        transpose4(y[k], lane);  // (every lane takes part in the exchange)
        int f, sb, n_s;
        if (!unit(k, f, sb, n_s)) continue;
        [[maybe_unused]] uint32_t E = 0;
        if constexpr (QUANT) {
            if (!cf) E = block_E<Q>(line_max(sb / MXB, f), ceil);  // (a strip along s lies in one block)
        }
        strip<Sd> o;
#pragma unroll
        for (int e = 0; e < SV; ++e) {
            float v = y[k][e];
            if constexpr (QUANT) {
                if (!cf) v = quant<Q>(v, E);
            } else {
                v = scale<float>(v, Ed::widen(old[k].e[e]), kind, false, alpha, beta);
            }
            if constexpr (SR)
                o.e[e] = Ed::narrow_sr(v, frow ? sr_bits(rh[k], uint32_t(S0) + uint32_t(sb + e), k1)
                                               : sr_bits(rh[e], uint32_t(F0) + uint32_t(f), k1));
            else
                o.e[e] = Ed::narrow(v);
        }
        store_at<Ed>(dst, f * ldd + sb, o, n_s, vd);
    }
}

// SR instances take the two 32-bit keys of the call's seed behind `ceil`; the others no argument more
template <typename Es, typename Ed, bool QUANT, bool SR, typename... Keys>
__global__ __launch_bounds__(SNT) void mx_kernel(const costa_scaled_op_t* __restrict__ ops,
                                                 const uint64_t* __restrict__ work, const char* src_base,
                                                 char* dst_base, const float* __restrict__ scalars, mx_side sa,
                                                 mx_side sc, int ceil, Keys... keys) {
    static_assert(sizeof...(Keys) == (SR ? 2 : 0), "k0, k1 with SR only");
    uint32_t k0 = 0, k1 = 0;
    if constexpr (SR) {
        const uint32_t kk[2] = {keys...};
        k0 = kk[0];
        k1 = kk[1];
    }
    uint32_t* red = nullptr;
    if constexpr (QUANT) {
        __shared__ uint32_t mx_red[MX_RED];
        red = mx_red;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tile = reinterpret_cast<float*>(smem);
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
    const float alpha = scalars[2 * slot];
    const float beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (tf == SBF && ts == SBS && (op.flags & vec_both) == vec_both)
        run_mx<Es, Ed, QUANT, SR, true>(sop, f0, s0, tf, ts, src_base, dst_base, alpha, beta, sa, sc, ceil != 0, tile,
                                        red, k0, k1);
    else
        run_mx<Es, Ed, QUANT, SR, false>(sop, f0, s0, tf, ts, src_base, dst_base, alpha, beta, sa, sc, ceil != 0, tile,
                                         red, k0, k1);
}

template <typename Es, typename Ed, bool QUANT>
void launch_inst(const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const char* src_base,
                 char* dst_base, const void* d_scalars, const mx_side& sa, const mx_side& sc, bool ceil,
                 const mx_sr* sr, hipStream_t stream) {
    if constexpr (QUANT) {
        if (sr) {
            launch_strip<&mx_kernel<Es, Ed, true, true, uint32_t, uint32_t>, sshape<float>::lds_bytes>(
                "MX", SNT, l, stream, d_ops, d_work, src_base, dst_base, static_cast<const float*>(d_scalars), sa, sc,
                int(ceil), sr->k0, sr->k1);
            return;
        }
    }
    launch_strip<&mx_kernel<Es, Ed, QUANT, false>, sshape<float>::lds_bytes>("MX", SNT, l, stream, d_ops, d_work,
                                                                            src_base, dst_base,
                                                                            static_cast<const float*>(d_scalars), sa,
                                                                            sc, int(ceil));
}

template <typename EQ>  // the codec of the pair's narrow type: q_e<Q>, q4_e or q6_e<T>
void launch_q(bool src_f, bool dst_f, const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
              const char* src_base, char* dst_base, const void* d_scalars, const mx_side& sa, const mx_side& sc,
              bool ceil, const mx_sr* sr, hipStream_t s) {
    if (src_f)
        launch_inst<f32_e, EQ, true>(d_ops, d_work, l, src_base, dst_base, d_scalars, sa, sc, ceil, sr, s);
    else if (dst_f)
        launch_inst<EQ, f32_e, false>(d_ops, d_work, l, src_base, dst_base, d_scalars, sa, sc, ceil, sr, s);
    else
        launch_inst<EQ, EQ, true>(d_ops, d_work, l, src_base, dst_base, d_scalars, sa, sc, ceil, sr, s);
}

}  // namespace

mx_sr mx_sr_keys(uint64_t seed) {
    return {fmix32(uint32_t(seed) ^ 0x9E3779B9u), fmix32(uint32_t(seed >> 32) ^ 0x85EBCA6Bu)};
}

uint32_t mx_sr_bits(uint64_t seed, int64_t i, int64_t j) {
    const mx_sr k = mx_sr_keys(seed);
    return fmix32((fmix32(uint32_t(i) ^ k.k0) + uint32_t(j)) ^ k.k1) >> 8;
}

bool mx_pair(costa_dtype_t src, costa_dtype_t dst) {
    return fp8_pair(src, dst) || packed_pair(src, dst);  // FLOAT -> Q, Q -> FLOAT, Q -> Q of one Q
}

void launch_mx(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* d_ops,
               const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
               const void* d_scalars, const mx_side& a_scales, const mx_side& c_scales, bool ceil, void* stream,
               const mx_sr* sr) {
    if (l.n_items <= 0) return;
    if (!mx_pair(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, std::string("costa: no MX kernel for ") + dtype_name(src_dtype) + " -> " +
                                       dtype_name(dst_dtype));
    const bool src_f = src_dtype == COSTA_FLOAT, dst_f = dst_dtype == COSTA_FLOAT;
    if ((a_scales.data != nullptr) == src_f || (c_scales.data != nullptr) == dst_f)
        throw error(COSTA_ERR_ARG, "costa: an MX launch needs a scale tensor exactly on its FP8 sides");
    if (sr && dst_f) throw error(COSTA_ERR_ARG, "costa: stochastic rounding needs a quantising MX launch (c_scales)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const costa_dtype_t nt = src_f ? dst_dtype : src_dtype;
    if (nt == COSTA_FP8_E4M3)
        launch_q<q_e<e4m3_t>>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, a_scales, c_scales, ceil, sr, s);
    else if (nt == COSTA_FP8_E5M2)
        launch_q<q_e<e5m2_t>>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, a_scales, c_scales, ceil, sr, s);
    else if (nt == COSTA_FP4_E2M1)
        launch_q<q4_e>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, a_scales, c_scales, ceil, sr, s);
    else if (nt == COSTA_FP6_E2M3)
        launch_q<q6_e<e2m3_t>>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, a_scales, c_scales, ceil, sr, s);
    else
        launch_q<q6_e<e3m2_t>>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, a_scales, c_scales, ceil, sr, s);
}

}  // namespace engine
}  // namespace costa
