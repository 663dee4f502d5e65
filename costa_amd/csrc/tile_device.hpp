// Device helpers shared by the tile kernels (tile_kernels.hip) and the converting kernels
// (convert_kernels.hip): element arithmetic in the reference's rounding order, 16-byte vector
// accesses, the cross-lane V x V transpose, and the 2-byte / 1-byte element types' widening and
// rounding (half_kernels.hip, fp8_kernels.hip, scaled_kernels.hip).  Everything is internal to the
// including file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "costa_hip.h"

#pragma clang fp contract(off)

namespace costa {
namespace engine {
namespace {

template <typename R>
struct cpx {
    R re, im;
};

// ---- element arithmetic, written out so the rounding sequence is explicit ----
template <typename T> __device__ __forceinline__ T e_mul(T a, T b) { return a * b; }
template <typename T> __device__ __forceinline__ T e_add(T a, T b) { return a + b; }
template <typename T> __device__ __forceinline__ T e_conj(T a) { return a; }
template <typename T> __device__ __forceinline__ T e_zero() { return T(0); }

// (a + i b)(c + i d): the reference's std::complex product as GCC compiles it (C99 Annex G):
// the naive (ac - bd, ad + bc) -- 4 products, 2 sums, no fma -- and, only when BOTH parts come
// out NaN, libgcc's __muldc3 / __mulsc3 recovery of infinities (GCC 11.4 libgcc2.c; restated in
// oracle/costa_oracle.c ANNEX_G_MUL and pinned to GCC there): an infinite factor is "boxed" to
// +-1 / +-0 with the other factor's NaNs zeroed, or, when a partial product overflowed, every
// NaN is zeroed; then the product is recomputed and scaled by infinity.  The branch is never
// taken on finite data: (inf + inf i)(1 + 0i) = inf + inf i, not NaN + NaN i.
// (the partial products are recomputed inside the rare branch rather than kept live: fewer
// registers on the common path)
template <typename R>
__device__ __attribute__((cold)) cpx<R> annex_g_recover(R a, R b, R c, R d) {
    const R one = R(1), zero = R(0), inf = __builtin_huge_val();
    const bool ovf = __builtin_isinf(a * c) || __builtin_isinf(b * d) || __builtin_isinf(a * d) ||
                     __builtin_isinf(b * c);
    bool recalc = false;
    if (__builtin_isinf(a) || __builtin_isinf(b)) {
        a = __builtin_copysign(__builtin_isinf(a) ? one : zero, a);
        b = __builtin_copysign(__builtin_isinf(b) ? one : zero, b);
        if (__builtin_isnan(c)) c = __builtin_copysign(zero, c);
        if (__builtin_isnan(d)) d = __builtin_copysign(zero, d);
        recalc = true;
    }
    if (__builtin_isinf(c) || __builtin_isinf(d)) {
        c = __builtin_copysign(__builtin_isinf(c) ? one : zero, c);
        d = __builtin_copysign(__builtin_isinf(d) ? one : zero, d);
        if (__builtin_isnan(a)) a = __builtin_copysign(zero, a);
        if (__builtin_isnan(b)) b = __builtin_copysign(zero, b);
        recalc = true;
    }
    if (!recalc && ovf) {
        if (__builtin_isnan(a)) a = __builtin_copysign(zero, a);
        if (__builtin_isnan(b)) b = __builtin_copysign(zero, b);
        if (__builtin_isnan(c)) c = __builtin_copysign(zero, c);
        if (__builtin_isnan(d)) d = __builtin_copysign(zero, d);
        recalc = true;
    }
    const R p = a * c, q = b * d, r = a * d, t = b * c;
    if (!recalc) return {p - q, r + t};
    return {inf * (p - q), inf * (r + t)};
}
#ifndef COSTA_ANNEX_G  // 0: naive complex products only (tuning builds: the recovery's cost)
#define COSTA_ANNEX_G 1
#endif
template <typename R>
__device__ __forceinline__ cpx<R> cmul(cpx<R> z, cpx<R> w) {
    const R x = z.re * w.re - z.im * w.im, y = z.re * w.im + z.im * w.re;
    if (COSTA_ANNEX_G && __builtin_expect(__builtin_isnan(x) && __builtin_isnan(y), 0))
        return annex_g_recover(z.re, z.im, w.re, w.im);
    return {x, y};
}
template <> __device__ __forceinline__ cpx<float> e_mul(cpx<float> a, cpx<float> b) { return cmul(a, b); }
template <> __device__ __forceinline__ cpx<double> e_mul(cpx<double> a, cpx<double> b) { return cmul(a, b); }
template <> __device__ __forceinline__ cpx<float> e_add(cpx<float> a, cpx<float> b) {
    return {a.re + b.re, a.im + b.im};
}
template <> __device__ __forceinline__ cpx<double> e_add(cpx<double> a, cpx<double> b) {
    return {a.re + b.re, a.im + b.im};
}
template <> __device__ __forceinline__ cpx<float> e_conj(cpx<float> a) { return {a.re, -a.im}; }
template <> __device__ __forceinline__ cpx<double> e_conj(cpx<double> a) { return {a.re, -a.im}; }
template <> __device__ __forceinline__ cpx<float> e_zero() { return {0.f, 0.f}; }
template <> __device__ __forceinline__ cpx<double> e_zero() { return {0.0, 0.0}; }

// g(x) for one element; `y` is the old destination value (read only for AXPBY)
template <typename T>
__device__ __forceinline__ T scale(T x, T y, uint32_t kind, bool conj, T alpha, T beta) {
    if (conj) x = e_conj(x);
    if (kind == COSTA_SCALE_ZERO) return e_zero<T>();
    if (kind == COSTA_SCALE_ALPHA) return e_mul(alpha, x);
    if (kind == COSTA_SCALE_AXPBY) return e_add(e_mul(beta, y), e_mul(alpha, x));
    return x;  // BITCOPY
}

// The same with the naive complex product only: `bad` is set when a product needs the Annex G
// recovery (both parts NaN), and the caller then redoes that vector with scale() out of the
// hot loop (run_tile): the recovery code stays off the register-hungry large shapes' main path
// (inlined per element it made the 1024-thread c64 shape spill to scratch).
template <typename T> struct is_cpx { static constexpr bool value = false; };
template <typename R> struct is_cpx<cpx<R>> { static constexpr bool value = true; };
// (a product whose parts are both NaN leaves both parts of the result NaN, beta * y + alpha * x
// included, so checking the result suffices; a NaN result for another reason is redone too,
// with the same outcome).  Costs cfg 4 (c128 'T', alpha, beta) ~3 %: 2.234 against 2.170 ms
// with naive products only (COSTA_ANNEX_G=0, profiles/r3/annex_ab.txt); storing unconditionally
// and fixing up afterwards would keep the old values live and spill.
template <typename T> __device__ __forceinline__ T e_mul_naive(T a, T b) { return a * b; }
template <typename R>
__device__ __forceinline__ cpx<R> e_mul_naive(cpx<R> z, cpx<R> w) {
    return {z.re * w.re - z.im * w.im, z.re * w.im + z.im * w.re};
}
template <typename T> __device__ __forceinline__ bool both_nan(const T&) { return false; }
template <typename R> __device__ __forceinline__ bool both_nan(const cpx<R>& v) {
    return COSTA_ANNEX_G && (v.re != v.re) & (v.im != v.im);
}
template <typename T>
__device__ __forceinline__ T scale_naive(T x, T y, uint32_t kind, bool conj, T alpha, T beta,
                                         bool& bad) {
    if (conj) x = e_conj(x);
    T r = x;  // BITCOPY
    if (kind == COSTA_SCALE_ZERO) r = e_zero<T>();
    else if (kind == COSTA_SCALE_ALPHA) r = e_mul_naive(alpha, x);
    else if (kind == COSTA_SCALE_AXPBY) r = e_add(e_mul_naive(beta, y), e_mul_naive(alpha, x));
    bad = bad | both_nan(r);
    return r;
}

// ---- cross-lane moves ----
[[maybe_unused]] __device__ __forceinline__ float shfl(float v, int l) { return __shfl(v, l); }
[[maybe_unused]] __device__ __forceinline__ int shfl(int v, int l) { return __shfl(v, l); }
[[maybe_unused]] __device__ __forceinline__ double shfl(double v, int l) { return __shfl(v, l); }
[[maybe_unused]] __device__ __forceinline__ cpx<float> shfl(cpx<float> v, int l) {
    return {__shfl(v.re, l), __shfl(v.im, l)};
}

// V elements = one 16-byte vector
template <typename T>
struct vec {
    static constexpr int V = 16 / int(sizeof(T));
    T e[V];
};
struct __attribute__((aligned(16))) raw16 {
    uint32_t w[4];
};

// 16-byte vector accesses of the tile kernels are non-temporal (`nt`): every byte of a
// transform is read once and written once, and on MI355X the nt policy moves such streams
// faster (tools/copy_ceiling.hip, profiles/r2/: a strided 2 GiB copy in 1 KiB column segments
// 6.37-6.49 TB/s with nt loads and stores against 6.02-6.23 without; cfg 2's transposed access
// pattern 6.27 against 5.73).
typedef uint32_t u32x4a __attribute__((ext_vector_type(4)));
// 16-byte loads need only dword alignment on gfx950 (global_load_dwordx4): sources of 4-byte
// elements off the 16-byte grid are read this way too (engine.cpp build_work marks them
// COSTA_TILE_VEC_SRC), so the load goes through a type that promises 4-byte alignment only
typedef uint32_t u32x4d __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ raw16 ld16(const void* p) {
    raw16 r;
    const u32x4d v = __builtin_nontemporal_load(reinterpret_cast<const u32x4d*>(p));
    __builtin_memcpy(&r, &v, 16);
    return r;
}
template <bool NT = true>
__device__ __forceinline__ void st16(void* p, const raw16& r) {
    if constexpr (NT) {
        u32x4a v;
        __builtin_memcpy(&v, &r, 16);
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4a*>(p));
    } else {
        *reinterpret_cast<raw16*>(p) = r;
    }
}

template <typename T, bool NT = true>
__device__ __forceinline__ void vload(vec<T>& out, const T* p, int n, bool vec_ok) {
    constexpr int V = vec<T>::V;
    if (vec_ok && n >= V) {
        raw16 r;
        if constexpr (NT) {
            r = ld16(p);
        } else {
            const u32x4d v = *reinterpret_cast<const u32x4d*>(p);
            __builtin_memcpy(&r, &v, 16);
        }
        __builtin_memcpy(&out, &r, 16);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < n) out.e[k] = p[k];
    }
}

template <typename T, bool NT = true>
__device__ __forceinline__ void vstore(T* p, const vec<T>& in, int n, bool vec_ok) {
    constexpr int V = vec<T>::V;
    if (vec_ok && n >= V) {
        raw16 r;
        __builtin_memcpy(&r, &in, 16);
        st16<NT>(p, r);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < n) p[k] = in.e[k];
    }
}

// Lanes k = 0..V-1 of an aligned group hold in[.] = row k of a V x V block; afterwards
// lane k holds column k.  Round r: every lane offers element (k - r) mod V and reads the
// offer of lane (k + r) mod V.  All indices are compile-time after unrolling.  The cross-lane
// read is a DPP quad permutation (a VALU move; V <= 4 lanes sit in one quad), not an LDS
// permute: the large shape spends its non-overlapped LDS time on the tile itself (the
// ds_bpermute form ran equally fast, 0.7063 ms both, with the LDS busier).
template <int V, int R>
constexpr int quad_ctrl() {  // quad_perm: lane q of each quad reads lane sel(q)
    int c = 0;
    for (int q = 0; q < 4; ++q) {
        const int base = q & ~(V - 1), k = q & (V - 1);
        c |= (base + ((k + R) & (V - 1))) << (2 * q);
    }
    return c;
}
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_move(T v) {
    static_assert(sizeof(T) % 4 == 0, "32-bit words");
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i)
        w[i] = uint32_t(__builtin_amdgcn_mov_dpp(int(w[i]), CTRL, 0xF, 0xF, true));
    T out;
    __builtin_memcpy(&out, w, sizeof(T));
    return out;
}
template <typename T, int R>
__device__ __forceinline__ void xround(const vec<T>& in, vec<T>& out, int lane) {
    constexpr int V = vec<T>::V;
    const int k = lane & (V - 1);
    const int give = (k - R) & (V - 1), from = (k + R) & (V - 1);
    T offer = in.e[0];
#pragma unroll
    for (int e = 1; e < V; ++e)
        if (e == give) offer = in.e[e];
    T got = offer;
    if constexpr (R != 0) got = dpp_move<quad_ctrl<V, R>()>(offer);
#pragma unroll
    for (int e = 0; e < V; ++e)
        if (e == from) out.e[e] = got;
}
// a[k] for a lane-dependent k in 0..3, as selects (a runtime-indexed vec<T> lives in scratch)
template <typename T>
__device__ __forceinline__ T sel4(int k, T a0, T a1, T a2, T a3) {
    return k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : a3;
}
template <typename T>
__device__ __forceinline__ vec<T> lane_transpose(const vec<T>& in, int lane) {
    constexpr int V = vec<T>::V;
    static_assert(V == 1 || V == 2 || V == 4, "one quad");
    vec<T> out;
    if constexpr (V == 1) {
        out = in;
    } else if constexpr (V == 2) {
        xround<T, 0>(in, out, lane);
        xround<T, 1>(in, out, lane);
    } else {
        // V = 4 (4-byte elements), every index compile-time: lane k rotates its row by k
        // (r[e] = in[(e + k) & 3]), so in round R every lane offers r[R] and lane k receives
        // in_{k-R}[k]; out[e] = g[(k - e) & 3] un-rotates (r13: the runtime-indexed form of
        // xround kept 144 bytes per lane in scratch and ran fp32 transposes at 3.3 TB/s)
        const int k = lane & 3;
        const T r0 = sel4(k, in.e[0], in.e[1], in.e[2], in.e[3]);
        const T r1 = sel4(k, in.e[1], in.e[2], in.e[3], in.e[0]);
        const T r2 = sel4(k, in.e[2], in.e[3], in.e[0], in.e[1]);
        const T r3 = sel4(k, in.e[3], in.e[0], in.e[1], in.e[2]);
        const T g0 = r0;
        const T g1 = dpp_move<quad_ctrl<4, 3>()>(r1);  // from lane (k - 1) & 3
        const T g2 = dpp_move<quad_ctrl<4, 2>()>(r2);  // from lane (k - 2) & 3
        const T g3 = dpp_move<quad_ctrl<4, 1>()>(r3);  // from lane (k - 3) & 3
        out.e[0] = sel4(k, g0, g1, g2, g3);
        out.e[1] = sel4(k, g3, g0, g1, g2);
        out.e[2] = sel4(k, g2, g3, g0, g1);
        out.e[3] = sel4(k, g1, g2, g3, g0);
    }
    return out;
}

// ---- narrow element types: shared by half_kernels.hip, fp8_kernels.hip and scaled_kernels.hip ----
// the two 2-byte types: raw bits, exact widening, rounding to nearest even
struct f16_t {
    static __device__ __forceinline__ float widen(uint16_t b) {
        _Float16 h;
        __builtin_memcpy(&h, &b, 2);
        return static_cast<float>(h);
    }
    static __device__ __forceinline__ uint16_t narrow(float x) {
        const _Float16 h = static_cast<_Float16>(x);  // RNE, +-inf on overflow, subnormals kept
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    }
};
struct bf16_t {
    static __device__ __forceinline__ float widen(uint16_t b) {
        const uint32_t u = uint32_t(b) << 16;
        float x;
        __builtin_memcpy(&x, &u, 4);
        return x;
    }
    static __device__ __forceinline__ uint16_t narrow(float x) {
#ifdef COSTA_HALF_BF16_INT  // (tuning builds: the integer form of the same rounding)
        uint32_t u;
        __builtin_memcpy(&u, &x, 4);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return uint16_t((u >> 16) | 0x40u);  // NaN stays NaN
        // round to nearest even on the 16 dropped bits; a carry out of the mantissa moves to the
        // exponent (the finite maximum goes to inf), subnormals round like everything else
        return uint16_t((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
#else
        const __bf16 h = static_cast<__bf16>(x);  // v_cvt_pk_bf16_f32: RNE, +-inf on overflow, subnormals kept
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
#endif
    }
};

__device__ __forceinline__ uint32_t f2u(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
__device__ __forceinline__ float u2f(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// The two 1-byte types: raw bits, exact widening, conversion as torch-CPU's .to(float8_*).
// narrow() rounds to nearest even on the dropped mantissa bits in integers (a carry out of the
// mantissa moves to the exponent); below the smallest normal the value is brought to the
// subnormals' fixed point by one exact fp32 addition (the sum's ulp is the subnormal step, so the
// addition itself rounds to nearest even, the tie below the smallest subnormal to zero).
template <int MB, int BIAS>
__device__ __forceinline__ uint32_t round_finite(uint32_t a) {  // |x| as fp32 bits, below the type's overflow
    constexpr int DROP = 23 - MB;
    constexpr uint32_t MIN_NORMAL = uint32_t(127 - BIAS + 1) << 23;
    constexpr uint32_t MAGIC = uint32_t(127 + DROP - BIAS + 1) << 23;  // 2^(subnormal step + 23)
    if (a < MIN_NORMAL) return f2u(u2f(a) + u2f(MAGIC)) - MAGIC;
    a += (uint32_t(BIAS - 127) << 23) + ((1u << (DROP - 1)) - 1u) + ((a >> DROP) & 1u);
    return a >> DROP;
}
// Stochastic rounding of the same |x| (costa_hip.h, "Stochastic rounding in the MX transforms"): U is
// the element's 24 random bits.  In the normal range the top DROP bits of U are added below the kept
// mantissa and the sum is truncated (a carry moves to the exponent); below the smallest normal |x| is
// brought to units of the subnormal step with 24 fraction bits -- an exact product with a power of
// two, below 2^(MB + 24), truncated by the conversion -- and U is added there.  A representable |x|
// has no dropped bits and keeps its code for every U.
template <int MB, int BIAS>
__device__ __forceinline__ uint32_t sr_finite(uint32_t a, uint32_t U) {
    constexpr int DROP = 23 - MB;
    constexpr uint32_t MIN_NORMAL = uint32_t(127 - BIAS + 1) << 23;
    constexpr uint32_t TO_FIXED = uint32_t(127 + 24 + BIAS - 1 + MB) << 23;  // 2^24 / the subnormal step
    if (a < MIN_NORMAL) return (uint32_t(u2f(a) * u2f(TO_FIXED)) + U) >> 24;
    return (a + (uint32_t(BIAS - 127) << 23) + (U >> (24 - DROP))) >> DROP;
}
struct e4m3_t {  // OCP e4m3fn: bias 7, no infinities, NaN = 0x7F / 0xFF, largest finite 448
    static __device__ __forceinline__ float widen(uint32_t b) {
        // the 7 magnitude bits read as binary16 (4-bit exponent in the low exponent bits) are the
        // value / 2^8, subnormals included
        const uint16_t hb = uint16_t((b & 0x7Fu) << 7);
        _Float16 h;
        __builtin_memcpy(&h, &hb, 2);
        const uint32_t m = (b & 0x7Fu) == 0x7Fu ? 0x7FC00000u : f2u(static_cast<float>(h) * 256.0f);
        return u2f(m | ((b & 0x80u) << 24));
    }
    static __device__ __forceinline__ uint32_t narrow(float x) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu, sign = (u >> 24) & 0x80u;
        // 480 = 1.875 * 2^8 and above (inf, NaN) -> NaN; (464, 480) rounds to the NaN code by itself
        if (a >= 0x43F00000u) return sign | 0x7Fu;
        return sign | round_finite<3, 7>(a);
    }
    // (the MX kernels clamp to 448 first: only a NaN reaches the first branch, and 448 + U never carries)
    static __device__ __forceinline__ uint32_t narrow_sr(float x, uint32_t U) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu, sign = (u >> 24) & 0x80u;
        if (a >= 0x43F00000u) return sign | 0x7Fu;
        return sign | sr_finite<3, 7>(a, U);
    }
};
struct e5m2_t {  // OCP e5m2: bias 15, the high byte of IEEE binary16
    static __device__ __forceinline__ float widen(uint32_t b) {
        const uint16_t hb = uint16_t((b & 0xFFu) << 8);
        _Float16 h;
        __builtin_memcpy(&h, &hb, 2);
        return static_cast<float>(h);
    }
    static __device__ __forceinline__ uint32_t narrow(float x) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu, sign = (u >> 24) & 0x80u;
        // NaN; 61440 = 1.875 * 2^15 and above -> +-inf ((57344, 61440) rounds by itself, the tie to inf)
        if (a >= 0x47700000u) return sign | (a > 0x7F800000u ? 0x7Fu : 0x7Cu);
        return sign | round_finite<2, 15>(a);
    }
    static __device__ __forceinline__ uint32_t narrow_sr(float x, uint32_t U) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu, sign = (u >> 24) & 0x80u;
        if (a >= 0x47700000u) return sign | (a > 0x7F800000u ? 0x7Fu : 0x7Cu);
        return sign | sr_finite<2, 15>(a, U);
    }
};

// The packed 4-bit type (costa_hip.h, "MXFP4"): one OCP e2m1 code, bit 3 the sign, bits 2..1 the
// exponent (bias 1), bit 0 the mantissa; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; no inf, no NaN.
struct e2m1_t {
    // w4: the 3 magnitude bits shifted to fp32's exponent / mantissa boundary are the value / 2^126
    // for the normal codes (2 .. 7); code 1 is the one subnormal, 0.5
    static __device__ __forceinline__ float widen(uint32_t c) {
        const uint32_t m = c & 7u;
        const uint32_t a = m >= 2u ? (m << 22) + (126u << 23) : m ? 0x3F000000u : 0u;
        return u2f(a | ((c & 8u) << 28));
    }
    // cvt4 of a finite t with |t| <= 6 (the caller clamps, so nothing overflows): round_finite with 1
    // mantissa bit and bias 1, whose round-to-nearest-even IS the tie rule of the type -- a tie goes to
    // the code whose mantissa bit is 0 (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4,
    // 5 -> 4); below 1.0 the one exact addition of 2^22 rounds to the subnormal step 0.5.  The sign bit
    // is always kept; NaN -> 0x0
    static __device__ __forceinline__ uint32_t narrow(float x) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu;
        if (a > 0x7F800000u) return 0u;
        return (u >> 28 & 8u) | round_finite<1, 1>(a);
    }
    static __device__ __forceinline__ uint32_t narrow_sr(float x, uint32_t U) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu;
        if (a > 0x7F800000u) return 0u;
        return (u >> 28 & 8u) | sr_finite<1, 1>(a, U);
    }
};

// The packed 6-bit types (costa_hip.h, "MXFP6"): one OCP FP6 code, bit 5 the sign, then the exponent
// and MB mantissa bits; no inf, no NaN.  e2m3: bias 1, subnormal step 1/8, largest 7.5; e3m2: bias 3,
// subnormal step 1/16, largest 28.
template <int MB, int BIAS>
struct fp6_t {
    // w6: the 5 magnitude bits shifted to fp32's exponent / mantissa boundary are the value /
    // 2^(127 - BIAS) for the normal codes; a subnormal code is its mantissa times the step (exact)
    static __device__ __forceinline__ float widen(uint32_t c) {
        const uint32_t m = c & 31u;
        const uint32_t a = m >= (1u << MB) ? (m << (23 - MB)) + (uint32_t(127 - BIAS) << 23)
                                           : f2u(float(m) * (1.0f / float(1 << (MB + BIAS - 1))));
        return u2f(a | ((c & 32u) << 26));
    }
    // cvt6 of a finite t with |t| <= fmax (the caller clamps, so nothing overflows): round_finite's
    // round-to-nearest-even on the dropped bits IS the tie rule of the type -- a tie goes to the code
    // whose mantissa is even, subnormals included (below the smallest normal one exact fp32 addition
    // rounds to the subnormal step).  The sign bit is always kept; NaN -> 0x00
    static __device__ __forceinline__ uint32_t narrow(float x) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu;
        if (a > 0x7F800000u) return 0u;
        return (u >> 26 & 32u) | round_finite<MB, BIAS>(a);
    }
    static __device__ __forceinline__ uint32_t narrow_sr(float x, uint32_t U) {
        const uint32_t u = f2u(x), a = u & 0x7FFFFFFFu;
        if (a > 0x7F800000u) return 0u;
        return (u >> 26 & 32u) | sr_finite<MB, BIAS>(a, U);
    }
};
using e2m3_t = fp6_t<3, 1>;
using e3m2_t = fp6_t<2, 3>;

}  // namespace
}  // namespace engine
}  // namespace costa
