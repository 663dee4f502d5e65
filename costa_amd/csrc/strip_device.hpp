// Device pieces shared by the kernel families that run 64 x 64 sub-tiles in strips of 4 elements
// (scaled_kernels.hip, mx_kernels.hip): the sub-tile's mapping constants, the element codecs, strip
// loads and stores, the staged tile's accessors, the 4 x 4 lane exchange and the unsigned-maximum
// helpers of the abs-max reductions.  Internal to the including file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "tile_device.hpp"

namespace costa {
namespace engine {
namespace {

#ifndef COSTA_SCALED_NT  // (overridden in tuning builds: 1024 threads on 128 x 128)
#define COSTA_SCALED_NT 256
#define COSTA_SCALED_BF 64
#define COSTA_SCALED_BS 64
#endif
constexpr int SNT = COSTA_SCALED_NT, SBF = COSTA_SCALED_BF, SBS = COSTA_SCALED_BS;  // threads, sub-tile (source fast x slow)
constexpr int SV = 4;                         // elements of a strip
constexpr int SLPC = SBF / SV;                // lanes per source column (load)
constexpr int SCPP = SNT / SLPC;              // source columns per load pass
constexpr int SPL = SBS / SCPP;               // load passes
constexpr int SNW = SNT / 64;                 // wavefronts
constexpr int SSW = 64;                       // s values of one store unit
constexpr int SQG = SBF / SV;                 // f slots (store units) per s chunk
constexpr int SUNITS = (SBS / SSW) * SQG;     // store units: 64 s x one f slot
constexpr int SPS = SUNITS / SNW;             // store passes
static_assert(SQG % SNW == 0 && SNT % SLPC == 0 && SBS % SCPP == 0 && SBS % SSW == 0 && SUNITS % SNW == 0, "mapping");

// ---- element codecs: storage type st, compute type ct, w() and cvt() ----
struct f32_e {
    using st = float;
    using ct = float;
    static __device__ __forceinline__ float widen(float x) { return x; }
    static __device__ __forceinline__ float narrow(float x) { return x; }
};
struct f64_e {
    using st = double;
    using ct = double;
    static __device__ __forceinline__ double widen(double x) { return x; }
    static __device__ __forceinline__ double narrow(double x) { return x; }
};
template <typename H>  // f16_t / bf16_t
struct h_e {
    using st = uint16_t;
    using ct = float;
    static __device__ __forceinline__ float widen(uint16_t b) { return H::widen(b); }
    static __device__ __forceinline__ uint16_t narrow(float x) { return H::narrow(x); }
};
template <typename Q>  // e4m3_t / e5m2_t
struct q_e {
    using st = uint8_t;
    using ct = float;
    static __device__ __forceinline__ float widen(uint8_t b) { return Q::widen(b); }
    static __device__ __forceinline__ uint8_t narrow(float x) { return uint8_t(Q::narrow(x)); }
    static __device__ __forceinline__ uint8_t narrow_sr(float x, uint32_t U) { return uint8_t(Q::narrow_sr(x, U)); }
};
// packed e2m1 (COSTA_FP4_E2M1): a strip<uint8_t> holds 4 unpacked codes, one per byte; two codes
// share a stored byte (load_strip4 / store_strip4 below)
struct q4_e {
    using st = uint8_t;
    using ct = float;
    static __device__ __forceinline__ float widen(uint8_t c) { return e2m1_t::widen(c); }
    static __device__ __forceinline__ uint8_t narrow(float x) { return uint8_t(e2m1_t::narrow(x)); }
    static __device__ __forceinline__ uint8_t narrow_sr(float x, uint32_t U) { return uint8_t(e2m1_t::narrow_sr(x, U)); }
};
// packed FP6 (COSTA_FP6_E2M3 / COSTA_FP6_E3M2; T = e2m3_t / e3m2_t): a strip<uint8_t> holds 4 unpacked
// codes, one per byte; four codes share three stored bytes (load_strip6 / store_strip6 below)
template <typename T>
struct q6_e {
    using st = uint8_t;
    using ct = float;
    static __device__ __forceinline__ float widen(uint8_t c) { return T::widen(c); }
    static __device__ __forceinline__ uint8_t narrow(float x) { return uint8_t(T::narrow(x)); }
    static __device__ __forceinline__ uint8_t narrow_sr(float x, uint32_t U) { return uint8_t(T::narrow_sr(x, U)); }
};
template <typename H>  // the FLOAT source of a FLOAT -> H pair: rounded to H first
struct f32_via {
    using st = float;
    using ct = float;
    static __device__ __forceinline__ float widen(float x) { return H::widen(H::narrow(x)); }
};

// ---- strips of 4 stored elements ----
template <typename S>
struct strip {
    S e[SV];
};
typedef uint32_t u32x2s __attribute__((ext_vector_type(2)));

// one vector access (fp64: two) where `vec_ok` (the side is aligned to the strip) and the strip is
// whole, else element by element; elements past n stay 0
template <typename S>
__device__ __forceinline__ strip<S> load_strip(const S* p, int n, bool vec_ok) {
    strip<S> out{};
    if (vec_ok && n >= SV) {
        if constexpr (sizeof(S) == 1) {
            const uint32_t v = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
            __builtin_memcpy(&out, &v, 4);
        } else if constexpr (sizeof(S) == 2) {
            const u32x2s v = __builtin_nontemporal_load(reinterpret_cast<const u32x2s*>(p));
            __builtin_memcpy(&out, &v, 8);
        } else if constexpr (sizeof(S) == 4) {
            const raw16 r = ld16(p);
            __builtin_memcpy(&out, &r, 16);
        } else {
            const raw16 a = ld16(p), b = ld16(p + 2);
            __builtin_memcpy(&out.e[0], &a, 16);
            __builtin_memcpy(&out.e[2], &b, 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < SV; ++k)
            if (k < n) out.e[k] = p[k];
    }
    return out;
}
template <typename S>
__device__ __forceinline__ void store_strip(S* p, const strip<S>& in, int n, bool vec_ok) {
    if (vec_ok && n >= SV) {
        if constexpr (sizeof(S) == 1) {
            uint32_t v;
            __builtin_memcpy(&v, &in, 4);
            __builtin_nontemporal_store(v, reinterpret_cast<uint32_t*>(p));
        } else if constexpr (sizeof(S) == 2) {
            u32x2s v;
            __builtin_memcpy(&v, &in, 8);
            __builtin_nontemporal_store(v, reinterpret_cast<u32x2s*>(p));
        } else if constexpr (sizeof(S) == 4) {
            raw16 r;
            __builtin_memcpy(&r, &in, 16);
            st16<true>(p, r);
        } else {
            raw16 a, b;
            __builtin_memcpy(&a, &in.e[0], 16);
            __builtin_memcpy(&b, &in.e[2], 16);
            st16<true>(p, a);
            st16<true>(p + 2, b);
        }
    } else {
#pragma unroll
        for (int k = 0; k < SV; ++k)
            if (k < n) p[k] = in.e[k];
    }
}

// a strip of 4 packed e2m1 codes: 2 bytes at p, the even element in bits 3..0.  One 2-byte access
// where `vec_ok` (p is 2-byte aligned on every line of the side) and the strip is whole, else a byte
// per pair of elements; n is even (the evenness rule), so a byte is read or written whole
__device__ __forceinline__ strip<uint8_t> load_strip4(const uint8_t* p, int n, bool vec_ok) {
    strip<uint8_t> out{};
    uint32_t v = 0;
    if (vec_ok && n >= SV) {
        v = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
    } else {
        if (n >= 2) v = p[0];
        if (n >= SV) v |= uint32_t(p[1]) << 8;
    }
#pragma unroll
    for (int k = 0; k < SV; ++k) out.e[k] = uint8_t(v >> (4 * k) & 15u);
    return out;
}
__device__ __forceinline__ void store_strip4(uint8_t* p, const strip<uint8_t>& in, int n, bool vec_ok) {
    const uint32_t lo = uint32_t(in.e[0] & 15u) | uint32_t(in.e[1] & 15u) << 4;
    const uint32_t hi = uint32_t(in.e[2] & 15u) | uint32_t(in.e[3] & 15u) << 4;
    if (vec_ok && n >= SV) {
        __builtin_nontemporal_store(uint16_t(lo | hi << 8), reinterpret_cast<uint16_t*>(p));
    } else {
        if (n >= 2) p[0] = uint8_t(lo);
        if (n >= SV) p[1] = uint8_t(hi);
    }
}

// a strip of 4 packed FP6 codes: one packing group, 3 bytes at p (any address), the first element in
// the lowest bits of w = c0 | c1 << 6 | c2 << 12 | c3 << 18.  Two non-temporal accesses: the low 2
// bytes at p through a type of alignment 1 (global memory takes a 2-byte access at an odd address; no
// alignment is asked of p) and the third byte at p + 2, so no byte outside the group is touched.  On
// an FP6 side a strip is whole or absent (the quad rule), so n < 4 moves nothing
typedef uint16_t u16_any __attribute__((aligned(1)));
__device__ __forceinline__ strip<uint8_t> load_strip6(const uint8_t* p, int n) {
    strip<uint8_t> out{};
    if (n >= SV) {
        const uint32_t w = uint32_t(__builtin_nontemporal_load(reinterpret_cast<const u16_any*>(p))) |
                           uint32_t(__builtin_nontemporal_load(p + 2)) << 16;
#pragma unroll
        for (int k = 0; k < SV; ++k) out.e[k] = uint8_t(w >> (6 * k) & 63u);
    }
    return out;
}
__device__ __forceinline__ void store_strip6(uint8_t* p, const strip<uint8_t>& in, int n) {
    if (n < SV) return;
    const uint32_t w = uint32_t(in.e[0] & 63u) | uint32_t(in.e[1] & 63u) << 6 | uint32_t(in.e[2] & 63u) << 12 |
                       uint32_t(in.e[3] & 63u) << 18;
    __builtin_nontemporal_store(uint16_t(w), reinterpret_cast<u16_any*>(p));
    __builtin_nontemporal_store(uint8_t(w >> 16), p + 2);
}

// a strip of the staged tile (compute type; 16-byte aligned)
template <typename C>
__device__ __forceinline__ void lds_put(C* p, const C (&w)[SV]) {
    constexpr int NQ = int(sizeof(C)) * SV / 16;
    raw16 r[NQ];
    __builtin_memcpy(&r[0], &w[0], sizeof(C) * SV);
#pragma unroll
    for (int i = 0; i < NQ; ++i) *(reinterpret_cast<raw16*>(p) + i) = r[i];
}
template <typename C>
__device__ __forceinline__ void lds_get(C (&w)[SV], const C* p) {
    constexpr int NQ = int(sizeof(C)) * SV / 16;
    raw16 r[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) r[i] = *(reinterpret_cast<const raw16*>(p) + i);
    __builtin_memcpy(&w[0], &r[0], sizeof(C) * SV);
}

// the 4 x 4 block of 4 lanes (lane_transpose; fp64: low and high words separately)
__device__ __forceinline__ void transpose4(float (&v)[SV], int lane) {
    vec<float> in;
#pragma unroll
    for (int e = 0; e < SV; ++e) in.e[e] = v[e];
    const vec<float> out = lane_transpose(in, lane);
#pragma unroll
    for (int e = 0; e < SV; ++e) v[e] = out.e[e];
}
__device__ __forceinline__ void transpose4(double (&v)[SV], int lane) {
    vec<uint32_t> lo, hi;
#pragma unroll
    for (int e = 0; e < SV; ++e) {
        uint64_t u;
        __builtin_memcpy(&u, &v[e], 8);
        lo.e[e] = uint32_t(u);
        hi.e[e] = uint32_t(u >> 32);
    }
    const vec<uint32_t> tl = lane_transpose(lo, lane), th = lane_transpose(hi, lane);
#pragma unroll
    for (int e = 0; e < SV; ++e) {
        const uint64_t u = uint64_t(tl.e[e]) | uint64_t(th.e[e]) << 32;
        __builtin_memcpy(&v[e], &u, 8);
    }
}

template <typename C>
struct sshape {
    static constexpr int P = SBF + 16 / int(sizeof(C));  // LDS row pitch (16 bytes of pad)
    static constexpr size_t lds_bytes = size_t(SBS) * P * sizeof(C);
};

// ---- abs-max reductions: unsigned maximum of absbits ----
template <typename C>
struct ubits {
    using type = uint32_t;
};
template <>
struct ubits<double> {
    using type = uint64_t;
};
template <typename C>
__device__ __forceinline__ typename ubits<C>::type absbits(C x) {
    using U = typename ubits<C>::type;
    U u;
    __builtin_memcpy(&u, &x, sizeof(U));
    return u & ~(U(1) << (8 * sizeof(U) - 1));
}
// lane (l + N) % 16 of the lane's own DPP row (every lane of the wavefront must be active)
template <int N>
__device__ __forceinline__ uint32_t row_ror(uint32_t v) {
    return uint32_t(__builtin_amdgcn_update_dpp(int(v), int(v), 0x120 + N, 0xf, 0xf, false));
}
template <int N>
__device__ __forceinline__ uint64_t row_ror(uint64_t v) {
    return uint64_t(row_ror<N>(uint32_t(v))) | uint64_t(row_ror<N>(uint32_t(v >> 32))) << 32;
}
template <typename U>
__device__ __forceinline__ U umax(U a, U b) {
    return a > b ? a : b;
}
template <typename U>
__device__ __forceinline__ U row_max16(U v) {
    v = umax(v, row_ror<8>(v));
    v = umax(v, row_ror<4>(v));
    v = umax(v, row_ror<2>(v));
    return umax(v, row_ror<1>(v));
}

}  // namespace
}  // namespace engine
}  // namespace costa
