// Converting tile kernels for CDNA4 (gfx950): the tile ops of a mixed-precision transform,
//   sub(C) = beta*sub(C) + alpha*op(convert(sub(A))),   fp64 <-> fp32, c128 <-> c64.
// An op reads elements of Ts and writes elements of Td:
//   copy mode       dst(f, s) = g(conv(src(f, s)))
//   transpose mode  dst(s, f) = g(conv(src(f, s)))
// conv is the C++ static_cast (round to nearest even, overflow to +-inf, fp32 subnormals kept,
// widening exact; complex per component); g is tile_kernel's scale<Td> with the same branches,
// contraction off, so the result equals, bit for bit, the same-type op run on a source that was
// converted first.  Scale kind BITCOPY means "convert only" here: g(x) = x after conv, never a
// byte copy.
//
// One kernel family, convert_kernel<Ts, Td>, driven like tile_kernel by a costa_tile_op_t array
// and (op << 32) | sub-tile work items; one workgroup runs one BF x BS sub-tile (conv_dims below:
// 128 x 128 elements and 1024 threads for the real pairs, 64 x 64 and 512 for the complex ones).
// A lane's unit of work is a strip of V elements along the source's fast dimension: one 16-byte
// vector of the wider type, 8 bytes of the narrower one.  Consecutive lanes then touch consecutive
// addresses on BOTH sides (16-byte accesses on the wide side, 8-byte on the narrow one); the
// conversion happens in registers.  (Strips of two wide vectors per 16-byte narrow vector were
// measured first: every wide-side instruction then touches alternate 16-byte pieces, and the
// widening stores ran at half the rate)
//   copy mode       no LDS: load strips, convert, scale, store strips
//   transpose mode  the sub-tile is staged in LDS in the NARROWER type (rows s, pitch BF + V: one
//                   8-byte strip of pad, conflict-free ds_write_b64 / ds_read_b64): narrowing ops
//                   convert before the LDS write, widening ops after the LDS read; V lanes
//                   exchange their V x V block (strip_transpose), so every lane stores V elements
//                   along the destination's fast dimension
// LDS: 128 x 130 x 4 = 66560 bytes for the real pairs, 64 x 65 x 8 = 33280 for the complex ones.
// Sub-tile remainders, ops below one strip and sides off their strip's alignment (VEC flag clear)
// take the guarded, element-wise form of the same loads and stores: same values, same result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "engine.hpp"
#include "strip_launch.hpp"
#include "tile_device.hpp"

#pragma clang fp contract(off)

namespace costa {
namespace engine {
namespace {

// the element conversion: static_cast, per component for complex
template <typename Td, typename Ts>
struct conv_t {
    static __device__ __forceinline__ Td of(Ts x) { return static_cast<Td>(x); }
};
template <typename Rd, typename Rs>
struct conv_t<cpx<Rd>, cpx<Rs>> {
    static __device__ __forceinline__ cpx<Rd> of(cpx<Rs> x) {
        return {static_cast<Rd>(x.re), static_cast<Rd>(x.im)};
    }
};
template <typename Td, typename Ts>
__device__ __forceinline__ Td conv(Ts x) {
    return conv_t<Td, Ts>::of(x);
}

// threads and sub-tile (elements along the source's fast x slow dimension) per size of the
// narrower element: the real pairs (4 bytes) and the complex pairs (8 bytes)
#ifndef COSTA_CONV_R_NT  // (overridden in tuning builds)
#define COSTA_CONV_R_NT 1024
#define COSTA_CONV_R_BF 128
#define COSTA_CONV_R_BS 128
#endif
#ifndef COSTA_CONV_C_NT
#define COSTA_CONV_C_NT 512
#define COSTA_CONV_C_BF 64
#define COSTA_CONV_C_BS 64
#endif
template <int NARROW_BYTES> struct conv_dims;
template <> struct conv_dims<4> {
    static constexpr int NT = COSTA_CONV_R_NT, BF = COSTA_CONV_R_BF, BS = COSTA_CONV_R_BS;
};
template <> struct conv_dims<8> {
    static constexpr int NT = COSTA_CONV_C_NT, BF = COSTA_CONV_C_BF, BS = COSTA_CONV_C_BS;
};

// sub-tile geometry (the load and store mappings of tile_kernels.hip `shape`, in strips)
template <typename Ts, typename Td>
struct cshape {
    static constexpr bool NARROW = sizeof(Ts) > sizeof(Td);
    using Tn = typename std::conditional<NARROW, Td, Ts>::type;  // the staged (narrower) type
    using Tw = typename std::conditional<NARROW, Ts, Td>::type;  // the wider type
    using dims = conv_dims<int(sizeof(Tn))>;
    static constexpr int NT = dims::NT;
    static constexpr int BF = dims::BF, BS = dims::BS;
    static constexpr int V = vec<Tw>::V;          // elements of a strip: 16 bytes wide, 8 narrow
    static constexpr int P = BF + V;              // LDS row pitch (one strip, 8 bytes, of pad)
    static constexpr int LPC = BF / V;            // lanes per source column (load)
    static constexpr int CPP = NT / LPC;          // source columns per load pass
    static constexpr int PL = BS / CPP;           // load passes
    static constexpr int NW = NT / 64;            // wavefronts
    static constexpr int SW = 64;                 // s values of one store unit
    static constexpr int QG = BF / V;             // f slots (store units) per s chunk
    static constexpr int UNITS = (BS / SW) * QG;  // store units: 64 s x one f slot
    static constexpr int PS = UNITS / NW;         // store passes
    static_assert(sizeof(Ts) == 2 * sizeof(Td) || 2 * sizeof(Ts) == sizeof(Td), "a 2:1 pair");
    static_assert(V * sizeof(Tn) == 8 && (V == 1 || V == 2), "8-byte strips of the narrower type");
    static_assert(NT % LPC == 0 && BS % CPP == 0 && BS % SW == 0 && UNITS % NW == 0, "mapping");
    static_assert(PL <= 32 && PS <= 32, "redo masks");
    static constexpr size_t lds_bytes = size_t(BS) * P * sizeof(Tn);
};

// N consecutive elements of T, 16 or 8 bytes: one vector access where `vec_ok` (the side is
// aligned to the strip) and the strip is whole, else element by element
template <typename T, int N>
struct strip {
    T e[N];
};
struct __attribute__((aligned(8))) raw8 {
    uint32_t w[2];
};
typedef uint32_t u32x2a __attribute__((ext_vector_type(2)));
template <typename T, int N>
__device__ __forceinline__ void sload(strip<T, N>& out, const T* p, int n, bool vec_ok) {
    static_assert(N * sizeof(T) == 16 || N * sizeof(T) == 8, "one vector");
    if (vec_ok && n >= N) {
        if constexpr (N * sizeof(T) == 16) {
            const raw16 r = ld16(p);
            __builtin_memcpy(&out, &r, 16);
        } else {
            const u32x2a v = __builtin_nontemporal_load(reinterpret_cast<const u32x2a*>(p));
            __builtin_memcpy(&out, &v, 8);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) out.e[k] = p[k];
    }
}
template <typename T, int N>
__device__ __forceinline__ void sstore(T* p, const strip<T, N>& in, int n, bool vec_ok) {
    static_assert(N * sizeof(T) == 16 || N * sizeof(T) == 8, "one vector");
    if (vec_ok && n >= N) {
        if constexpr (N * sizeof(T) == 16) {
            raw16 r;
            __builtin_memcpy(&r, &in, 16);
            st16<true>(p, r);
        } else {
            u32x2a v;
            __builtin_memcpy(&v, &in, 8);
            __builtin_nontemporal_store(v, reinterpret_cast<u32x2a*>(p));
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) p[k] = in.e[k];
    }
}
// Lanes k = 0..N-1 of an aligned group hold row k of an N x N block; afterwards lane k holds
// column k (N = 2: one DPP move inside the quad; N = 1: nothing to do)
template <typename T, int N>
__device__ __forceinline__ strip<T, N> strip_transpose(const strip<T, N>& in, int lane) {
    if constexpr (N == 1) {
        return in;
    } else {
        static_assert(N == 2, "pairs of lanes");
        const bool odd = lane & 1;
        const T got = dpp_move<quad_ctrl<2, 1>()>(odd ? in.e[0] : in.e[1]);  // the partner's offer
        strip<T, N> out;
        out.e[0] = odd ? got : in.e[0];
        out.e[1] = odd ? in.e[1] : got;
        return out;
    }
}

// One sub-tile.  FULL: a whole BF x BS sub-tile with both VEC flags, every guard folds away.
template <typename Ts, typename Td, bool FULL>
__device__ __forceinline__ void run_convert(const costa_tile_op_t& op, int f0, int s0, int tf_, int ts_,
                                            const char* src_base, char* dst_base, Td alpha, Td beta,
                                            typename cshape<Ts, Td>::Tn* tile) {
    using S = cshape<Ts, Td>;
    using Tn = typename S::Tn;
    constexpr int V = S::V, P = S::P;
    const int tf = FULL ? S::BF : tf_;
    const int ts = FULL ? S::BS : ts_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool conj = flags & COSTA_TILE_CONJ;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const bool vd = FULL || (flags & COSTA_TILE_VEC_DST);
    const int64_t lds = op.lds, ldd = op.ldd;
    const Ts* src = reinterpret_cast<const Ts*>(src_base + op.src) + int64_t(s0) * lds + f0;

    // ---- load phase: lane -> (strip along f, column s); all loads issued first
    const int lf = (int(threadIdx.x) % S::LPC) * V;
    const int c0 = int(threadIdx.x) / S::LPC;
    auto col_of = [&](int k) { return c0 + k * S::CPP; };
    const int nf_lane = FULL ? V : tf - lf;  // elements of this lane's strip inside the sub-tile
    strip<Ts, V> x[S::PL];
#pragma unroll
    for (int k = 0; k < S::PL; ++k) {
        const int s = col_of(k);
        if (FULL || (nf_lane > 0 && s < ts)) sload(x[k], src + s * lds + lf, nf_lane, vs);
    }

    if (!(flags & COSTA_TILE_TRANSPOSE)) {
        // ---- copy mode: dst(f, s) = g(conv(src(f, s))), no LDS
        Td* dst = reinterpret_cast<Td*>(dst_base + op.dst) + int64_t(s0) * ldd + f0;
        strip<Td, V> y[S::PL];  // beta != 0: every old value is requested before the first store
        if (kind == COSTA_SCALE_AXPBY) {
#pragma unroll
            for (int k = 0; k < S::PL; ++k) {
                const int s = col_of(k);
                if (FULL || (nf_lane > 0 && s < ts)) sload(y[k], dst + s * ldd + lf, nf_lane, vd);
            }
        }
        uint32_t redo = 0;  // complex strips left for the Annex G path (bit k: strip k)
#pragma unroll
        for (int k = 0; k < S::PL; ++k) {
            const int s = col_of(k);
            if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
            strip<Td, V> o;
            bool bad = false;
#pragma unroll
            for (int e = 0; e < V; ++e)
                o.e[e] = scale_naive(conv<Td>(x[k].e[e]),
                                     kind == COSTA_SCALE_AXPBY ? y[k].e[e] : e_zero<Td>(), kind, conj,
                                     alpha, beta, bad);
            if (is_cpx<Td>::value && bad) {
                redo |= 1u << k;
                continue;
            }
            sstore(dst + s * ldd + lf, o, nf_lane, vd);
        }
        if constexpr (is_cpx<Td>::value) {
            // strips whose naive products needed the recovery: source and (not yet written)
            // destination are read again and every element goes through scale()
            if (__builtin_expect(redo != 0, 0)) {
#pragma unroll 1
                for (int k = 0; k < S::PL; ++k) {
                    if (!((redo >> k) & 1u)) continue;
                    const int s = col_of(k);
                    const Ts* a = src + s * lds + lf;
                    Td* d = dst + s * ldd + lf;
                    const int n = FULL ? V : min(V, nf_lane);
#pragma unroll 1
                    for (int e = 0; e < n; ++e)
                        d[e] = scale(conv<Td>(a[e]), kind == COSTA_SCALE_AXPBY ? d[e] : e_zero<Td>(),
                                     kind, conj, alpha, beta);
                }
            }
        }
        return;
    }

    // ---- transpose mode: dst(s, f) = g(conv(src(f, s))) through LDS, staged in the narrower type
    Td* dst = reinterpret_cast<Td*>(dst_base + op.dst) + int64_t(f0) * ldd + s0;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    constexpr int SW = S::SW, QG = S::QG;
    // store unit k of this lane: 64 s values of one f slot; after the lane exchange lane
    // (base + j) stores f = q*V + j for s = sc*SW + base .. + V-1
    auto unit = [&](int k, int& f, int& sb, int& n) {
        const int u = wave + S::NW * k;
        const int sc = u / QG, q = u % QG;
        const int j = lane & (V - 1);
        f = q * V + j;
        sb = sc * SW + (lane - j);
        n = FULL ? V : ts - sb;
        return FULL || (f < tf && n > 0);
    };
    // beta != 0: the old destination values are requested now, with the source loads in flight
    strip<Td, V> old[S::PS];
    if (kind == COSTA_SCALE_AXPBY) {
#pragma unroll
        for (int k = 0; k < S::PS; ++k) {
            int f, sb, n;
            if (unit(k, f, sb, n)) sload(old[k], dst + f * ldd + sb, n, vd);
        }
    }
#pragma unroll
    for (int k = 0; k < S::PL; ++k) {
        const int s = col_of(k);
        if (FULL || (nf_lane > 0 && s < ts)) {  // partial strips: the tail is junk, never stored
            strip<Tn, V> t;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if constexpr (S::NARROW) t.e[e] = conv<Td>(x[k].e[e]);
                else t.e[e] = x[k].e[e];
            }
            raw8 r;
            __builtin_memcpy(&r, &t, 8);
            *reinterpret_cast<raw8*>(tile + s * P + lf) = r;
        }
    }
    __syncthreads();

    strip<Tn, V> y[S::PS];
#pragma unroll
    for (int k = 0; k < S::PS; ++k) {
        const int u = wave + S::NW * k;
        const int sc = u / QG, q = u % QG;
        const int s = sc * SW + lane;
        if (FULL || (s < ts && q * V < tf)) {
            const raw8 r = *reinterpret_cast<const raw8*>(tile + s * P + q * V);
            __builtin_memcpy(&y[k], &r, 8);
        }
    }
    uint32_t redo = 0;  // complex store units left for the Annex G path (bit k: unit k)
#pragma unroll
    for (int k = 0; k < S::PS; ++k) {
        const strip<Tn, V> t = strip_transpose(y[k], lane);
        int f, sb, n;
        if (!unit(k, f, sb, n)) continue;
        strip<Td, V> o;
        bool bad = false;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            Td v;
            if constexpr (S::NARROW) v = t.e[e];
            else v = conv<Td>(t.e[e]);
            o.e[e] = scale_naive(v, kind == COSTA_SCALE_AXPBY ? old[k].e[e] : e_zero<Td>(), kind, conj,
                                 alpha, beta, bad);
        }
        if (is_cpx<Td>::value && bad) {
            redo |= 1u << k;
            continue;
        }
        sstore(dst + f * ldd + sb, o, n, vd);
    }
    if constexpr (is_cpx<Td>::value) {
        // units whose naive products needed the recovery: element e of the unit is source row
        // sb + e, column f of the staged tile; its old value is still in the destination
        if (__builtin_expect(redo != 0, 0)) {
#pragma unroll 1
            for (int k = 0; k < S::PS; ++k) {
                if (!((redo >> k) & 1u)) continue;
                int f, sb, n;
                unit(k, f, sb, n);
                Td* d = dst + f * ldd + sb;
                n = FULL ? V : min(V, n);
#pragma unroll 1
                for (int e = 0; e < n; ++e) {
                    Td v;
                    if constexpr (S::NARROW) v = tile[(sb + e) * P + f];
                    else v = conv<Td>(tile[(sb + e) * P + f]);
                    d[e] = scale(v, kind == COSTA_SCALE_AXPBY ? d[e] : e_zero<Td>(), kind, conj, alpha,
                                 beta);
                }
            }
        }
    }
}

template <typename Ts, typename Td>
__global__ __launch_bounds__((cshape<Ts, Td>::NT)) void convert_kernel(const costa_tile_op_t* __restrict__ ops,
                                                      const uint64_t* __restrict__ work,
                                                      const char* src_base, char* dst_base,
                                                      const Td* __restrict__ scalars) {
    using S = cshape<Ts, Td>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typename S::Tn* tile = reinterpret_cast<typename S::Tn*>(smem);
    // which sub-tile of which op (wave-uniform: scalar loads)
    const uint64_t w = work[blockIdx.x];
    const costa_tile_op_t op = ops[w >> 32];
    const uint32_t sub = uint32_t(w);
    const int nbf = (op.nf + S::BF - 1) / S::BF;
    const int f0 = int(sub % uint32_t(nbf)) * S::BF;
    const int s0 = int(sub / uint32_t(nbf)) * S::BS;
    const int tf = min(S::BF, op.nf - f0);
    const int ts = min(S::BS, op.ns - s0);
    const uint32_t slot = op.flags >> COSTA_SLOT_SHIFT;
    const Td alpha = scalars[2 * slot];
    const Td beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (tf == S::BF && ts == S::BS && (op.flags & vec_both) == vec_both)
        run_convert<Ts, Td, true>(op, f0, s0, tf, ts, src_base, dst_base, alpha, beta, tile);
    else
        run_convert<Ts, Td, false>(op, f0, s0, tf, ts, src_base, dst_base, alpha, beta, tile);
}

template <typename Ts, typename Td>
void launch_pair(const costa_tile_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
                 const char* src_base, char* dst_base, const void* d_scalars, hipStream_t stream) {
    using S = cshape<Ts, Td>;
    launch_strip<&convert_kernel<Ts, Td>, S::lds_bytes>("convert", S::NT, l, stream, d_ops, d_work, src_base,
                                                        dst_base, static_cast<const Td*>(d_scalars));
}

void wide_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs) {
    const bool cplx = dtype_is_complex(src);
    *bf = cplx ? conv_dims<8>::BF : conv_dims<4>::BF;
    *bs = cplx ? conv_dims<8>::BS : conv_dims<4>::BS;
}

void launch_wide(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* d_ops,
                 const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                 const void* d_scalars, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (src_dtype == COSTA_DOUBLE)
        launch_pair<double, float>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else if (src_dtype == COSTA_FLOAT)
        launch_pair<float, double>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else if (src_dtype == COSTA_CDOUBLE)
        launch_pair<cpx<double>, cpx<float>>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else
        launch_pair<cpx<float>, cpx<double>>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
}

}  // namespace

// (reached through the pair table of engine.cpp: wide_pair(src, dst) holds)
pair_family wide_family() { return {wide_pair, wide_subtile, launch_wide}; }

}  // namespace engine
}  // namespace costa
