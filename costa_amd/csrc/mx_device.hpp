// Device pieces shared by the MX kernel files (mx_kernels.hip, mx_dual_kernels.hip): the limits of the
// OCP floor rule per destination type, a block's E and the quantising product, the half-row maximum of
// the blocks-along-f reduction, the hash of stochastic rounding and the element-offset / strip access
// of the packed sides.  Register arithmetic only: nothing here touches LDS or memory but load_at /
// store_at, which are the strip accesses of strip_device.hpp at a side's own offset.  Internal to the
// including file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "strip_device.hpp"
#include "tile_device.hpp"

namespace costa {
namespace engine {
namespace {

static_assert(SLPC == 16 && SBF == 64 && SBS == 64 && SNW == 4 && SPL == 4,
              "the MX block reduction is mapped to 64 x 64 sub-tiles of 256 threads");
constexpr int MXB = 32;                   // elements of a block
constexpr int MX_RED = SNW * 2 * SBF;     // words of the reduction's LDS array

// the limits of the OCP floor rule per destination type
template <typename Q>
struct qlim;
template <>
struct qlim<e4m3_t> {
    static constexpr uint32_t emax = 8, fmax = 0x43E00000u;  // 448
};
template <>
struct qlim<e5m2_t> {
    static constexpr uint32_t emax = 15, fmax = 0x47600000u;  // 57344
};
template <>
struct qlim<e2m1_t> {
    static constexpr uint32_t emax = 2, fmax = 0x40C00000u;  // 6
};
template <>
struct qlim<e2m3_t> {
    static constexpr uint32_t emax = 2, fmax = 0x40F00000u;  // 7.5
};
template <>
struct qlim<e3m2_t> {
    static constexpr uint32_t emax = 4, fmax = 0x41E00000u;  // 28
};
template <typename E>
struct q_of {
    using type = e4m3_t;  // (unused for FLOAT destinations)
};
template <typename Q>
struct q_of<q_e<Q>> {
    using type = Q;
};
template <>
struct q_of<q4_e> {
    using type = e2m1_t;
};

template <typename T>
struct q_of<q6_e<T>> {
    using type = T;
};
template <typename E>
struct is_q6 : std::false_type {};
template <typename T>
struct is_q6<q6_e<T>> : std::true_type {};

// element offset -> offset in storage units of the side (packed e2m1: two elements per byte, `at`
// is even there; packed FP6: four elements per three bytes, `at` is a multiple of 4 there)
template <typename E>
__device__ __forceinline__ int64_t elems(int64_t at) {
    if constexpr (std::is_same<E, q4_e>::value) return at >> 1;
    if constexpr (is_q6<E>::value) return (at >> 2) * 3;
    return at;
}
// the strip at element offset `at` from p
template <typename E>
__device__ __forceinline__ strip<typename E::st> load_at(const typename E::st* p, int64_t at, int n, bool vec_ok) {
    if constexpr (std::is_same<E, q4_e>::value) return load_strip4(p + (at >> 1), n, vec_ok);
    if constexpr (is_q6<E>::value) return load_strip6(p + (at >> 2) * 3, n);
    return load_strip(p + at, n, vec_ok);
}
template <typename E>
__device__ __forceinline__ void store_at(typename E::st* p, int64_t at, const strip<typename E::st>& v, int n,
                                         bool vec_ok) {
    if constexpr (std::is_same<E, q4_e>::value)
        store_strip4(p + (at >> 1), v, n, vec_ok);
    else if constexpr (is_q6<E>::value)
        store_strip6(p + (at >> 2) * 3, v, n);
    else
        store_strip(p + at, v, n, vec_ok);
}

__device__ __forceinline__ float pow2(uint32_t E) {
    return u2f(E == 0 ? 0x00400000u : E == 255 ? 0x7FC00000u : E << 23);
}
template <typename Q>
__device__ __forceinline__ uint32_t block_E(uint32_t amax, bool ceil) {
    const uint32_t e = amax >> 23;
    if (e == 255) return 255;
    uint32_t E = e > qlim<Q>::emax ? e - qlim<Q>::emax : 0u;
    if (ceil && E < 254 && u2f(amax) * pow2(254 - E) > u2f(qlim<Q>::fmax)) ++E;
    return E;
}
template <typename Q>
__device__ __forceinline__ float quant(float v, uint32_t E) {
    if (E == 255) return u2f(0x7FC00000u);
    const float t = v * pow2(254 - E), fm = u2f(qlim<Q>::fmax);
    return t > fm ? fm : t < -fm ? -fm : t;  // (a NaN stays)
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_self(uint32_t v) {
    return uint32_t(__builtin_amdgcn_update_dpp(int(v), int(v), CTRL, 0xf, 0xf, false));
}
// the maximum over the 8 lanes of the lane's half DPP row (every lane of the wavefront active)
__device__ __forceinline__ uint32_t half_row_max(uint32_t v) {
    v = umax(v, dpp_self<0xB1>(v));    // quad_perm [1, 0, 3, 2]
    v = umax(v, dpp_self<0x4E>(v));    // quad_perm [2, 3, 0, 1]
    return umax(v, dpp_self<0x141>(v));  // row_half_mirror: the other quad
}

// ---- stochastic rounding (costa_hip.h, "Stochastic rounding in the MX transforms") ----
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}
// U(seed, i, j) from the row's inner hash r = fmix32(uint32(i) ^ k0)
__device__ __forceinline__ uint32_t sr_bits(uint32_t r, uint32_t j, uint32_t k1) { return fmix32((r + j) ^ k1) >> 8; }

}  // namespace
}  // namespace engine
}  // namespace costa
