// Half-precision tile kernels for CDNA4 (gfx950): the tile ops of transforms whose A or C holds a
// 2-byte element type H (IEEE binary16 or bfloat16, raw bits),
//   H -> H (one H), FLOAT -> H, H -> FLOAT      (costa_hip.h, "Half precision").
// With w() the exact widening to fp32, cvt() the conversion fp32 -> H (round to nearest even,
// overflow to +-inf, subnormals kept) and g() tile_kernel's scale<float> (same branches,
// contraction off), an op computes, for its source element x and old destination value y,
//   H -> H        cvt(g(w(x), w(y)))         scale kind BITCOPY: the bits of x (a byte copy)
//   FLOAT -> H    the same on cvt(x): the source is rounded to H first
//   H -> FLOAT    g(w(x), y)
// in copy mode dst(f, s), in transpose mode dst(s, f): fp32 arithmetic, one rounding at the store.
//
// One kernel family, half_kernel<H, SRC_F, DST_F>, driven exactly like convert_kernel by a
// costa_tile_op_t array and (op << 32) | sub-tile work items; one workgroup of 1024 threads runs
// one 128 x 128 sub-tile.  A lane's unit of work is a strip of 4 elements along the source's fast
// dimension: 8 bytes on a 2-byte side, 16 on an fp32 side, so consecutive lanes touch consecutive
// addresses on both sides.  Whatever the pair, the source strip is brought to H at once (FLOAT
// sources are rounded here), so every later stage handles 8-byte strips of H.
//   copy mode       no LDS: load strips, compute, store strips
//   transpose mode  the sub-tile is staged in LDS in H (rows s, pitch 128 + 4 elements: one 8-byte
//                   strip of pad, so the ds_write_b64 of consecutive lanes and the ds_read_b64 at
//                   a stride of 66 dwords are both conflict-free); 4 lanes then exchange their
//                   4 x 4 block with DPP quad permutations (lane_transpose, compile-time register
//                   indices only), so every lane stores 4 elements along the destination's fast
//                   dimension
// LDS: 128 x 132 x 2 = 33792 bytes.  Old destination values (beta != 0) are requested before the
// first wait.  Whole sub-tiles with both VEC flags take the FULL path, where every guard folds
// away; sub-tile remainders, ops below one strip and sides off their strip's alignment (VEC flag
// clear) take the guarded, element-wise form of the same loads and stores: same values.
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

#ifndef COSTA_HALF_NT  // (overridden in tuning builds)
#define COSTA_HALF_NT 1024
#define COSTA_HALF_BF 128
#define COSTA_HALF_BS 128
#endif
constexpr int HNT = COSTA_HALF_NT, HBF = COSTA_HALF_BF, HBS = COSTA_HALF_BS;  // threads, sub-tile (source fast x slow)
constexpr int HV = 4;                            // elements of a strip
constexpr int HP = HBF + HV;                     // LDS row pitch (elements of H)
constexpr int HLPC = HBF / HV;                   // lanes per source column (load)
constexpr int HCPP = HNT / HLPC;                 // source columns per load pass
constexpr int HPL = HBS / HCPP;                  // load passes
constexpr int HNW = HNT / 64;                    // wavefronts
constexpr int HSW = 64;                          // s values of one store unit
constexpr int HQG = HBF / HV;                    // f slots (store units) per s chunk
constexpr int HUNITS = (HBS / HSW) * HQG;        // store units: 64 s x one f slot
constexpr int HPS = HUNITS / HNW;                // store passes
static_assert(HNT % HLPC == 0 && HBS % HCPP == 0 && HBS % HSW == 0 && HUNITS % HNW == 0, "mapping");
constexpr size_t kHalfLds = size_t(HBS) * HP * 2;

// (f16_t / bf16_t, the two 2-byte types: tile_device.hpp)
// a strip of 4 elements of H (8 bytes) / of fp32 (16 bytes)
struct hstrip {
    uint16_t e[HV];
};
struct fstrip {
    float e[HV];
};
typedef uint32_t u32x2h __attribute__((ext_vector_type(2)));

// one vector access where `vec_ok` (the side is aligned to the strip) and the strip is whole, else
// element by element; elements past n stay 0
__device__ __forceinline__ hstrip load_h(const uint16_t* p, int n, bool vec_ok) {
    hstrip out = {{0, 0, 0, 0}};
    if (vec_ok && n >= HV) {
        const u32x2h v = __builtin_nontemporal_load(reinterpret_cast<const u32x2h*>(p));
        __builtin_memcpy(&out, &v, 8);
    } else {
#pragma unroll
        for (int k = 0; k < HV; ++k)
            if (k < n) out.e[k] = p[k];
    }
    return out;
}
__device__ __forceinline__ fstrip load_f(const float* p, int n, bool vec_ok) {
    fstrip out = {{0.f, 0.f, 0.f, 0.f}};
    if (vec_ok && n >= HV) {
        const raw16 r = ld16(p);
        __builtin_memcpy(&out, &r, 16);
    } else {
#pragma unroll
        for (int k = 0; k < HV; ++k)
            if (k < n) out.e[k] = p[k];
    }
    return out;
}
__device__ __forceinline__ void store_h(uint16_t* p, const hstrip& in, int n, bool vec_ok) {
    if (vec_ok && n >= HV) {
        u32x2h v;
        __builtin_memcpy(&v, &in, 8);
        __builtin_nontemporal_store(v, reinterpret_cast<u32x2h*>(p));
    } else {
#pragma unroll
        for (int k = 0; k < HV; ++k)
            if (k < n) p[k] = in.e[k];
    }
}
__device__ __forceinline__ void store_f(float* p, const fstrip& in, int n, bool vec_ok) {
    if (vec_ok && n >= HV) {
        raw16 r;
        __builtin_memcpy(&r, &in, 16);
        st16<true>(p, r);
    } else {
#pragma unroll
        for (int k = 0; k < HV; ++k)
            if (k < n) p[k] = in.e[k];
    }
}

// The pair's element types and the per-strip steps.  SRC_F / DST_F: that side holds fp32.
template <typename H, bool SRC_F, bool DST_F>
struct hpair {
    using Ts = typename std::conditional<SRC_F, float, uint16_t>::type;
    using Td = typename std::conditional<DST_F, float, uint16_t>::type;
    using dstrip = typename std::conditional<DST_F, fstrip, hstrip>::type;
    static_assert(!(SRC_F && DST_F), "one side at least holds the 2-byte type");

    // the source strip as H: FLOAT sources are rounded to H here
    static __device__ __forceinline__ hstrip load_src(const Ts* p, int n, bool vec_ok) {
        if constexpr (SRC_F) {
            const fstrip x = load_f(p, n, vec_ok);
            hstrip h;
#pragma unroll
            for (int e = 0; e < HV; ++e) h.e[e] = H::narrow(x.e[e]);
            return h;
        } else {
            return load_h(p, n, vec_ok);
        }
    }
    static __device__ __forceinline__ dstrip load_dst(const Td* p, int n, bool vec_ok) {
        if constexpr (DST_F) return load_f(p, n, vec_ok);
        else return load_h(p, n, vec_ok);
    }
    static __device__ __forceinline__ void store_dst(Td* p, const dstrip& o, int n, bool vec_ok) {
        if constexpr (DST_F) store_f(p, o, n, vec_ok);
        else store_h(p, o, n, vec_ok);
    }
    // one element: x as H bits, y the old destination value (read only for AXPBY)
    static __device__ __forceinline__ Td element(uint16_t x, Td y, uint32_t kind, float alpha, float beta) {
        if constexpr (DST_F) {
            return scale<float>(H::widen(x), y, kind, false, alpha, beta);
        } else {
            if (kind == COSTA_SCALE_BITCOPY) return x;  // a byte copy (FLOAT sources: cvt(x))
            return H::narrow(scale<float>(H::widen(x), H::widen(y), kind, false, alpha, beta));
        }
    }
    static __device__ __forceinline__ dstrip compute(const hstrip& x, const dstrip& y, uint32_t kind,
                                                     float alpha, float beta) {
        dstrip o;
#pragma unroll
        for (int e = 0; e < HV; ++e) o.e[e] = element(x.e[e], y.e[e], kind, alpha, beta);
        return o;
    }
};

// One sub-tile.  FULL: a whole 128 x 128 sub-tile with both VEC flags, every guard folds away.
template <typename H, bool SRC_F, bool DST_F, bool FULL>
__device__ __forceinline__ void run_half(const costa_tile_op_t& op, int f0, int s0, int tf_, int ts_,
                                         const char* src_base, char* dst_base, float alpha, float beta,
                                         uint16_t* tile) {
    using PR = hpair<H, SRC_F, DST_F>;
    using Ts = typename PR::Ts;
    using Td = typename PR::Td;
    using dstrip = typename PR::dstrip;
    const int tf = FULL ? HBF : tf_;
    const int ts = FULL ? HBS : ts_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const bool vd = FULL || (flags & COSTA_TILE_VEC_DST);
    const int64_t lds = op.lds, ldd = op.ldd;
    const Ts* src = reinterpret_cast<const Ts*>(src_base + op.src) + int64_t(s0) * lds + f0;

    // ---- load phase: lane -> (strip along f, column s); all loads issued first
    const int lf = (int(threadIdx.x) % HLPC) * HV;
    const int c0 = int(threadIdx.x) / HLPC;
    const int nf_lane = FULL ? HV : tf - lf;  // elements of this lane's strip inside the sub-tile
    hstrip x[HPL];
#pragma unroll
    for (int k = 0; k < HPL; ++k) {
        const int s = c0 + k * HCPP;
        if (FULL || (nf_lane > 0 && s < ts)) x[k] = PR::load_src(src + s * lds + lf, nf_lane, vs);
        else x[k] = hstrip{{0, 0, 0, 0}};
    }

    if (!(flags & COSTA_TILE_TRANSPOSE)) {
        // ---- copy mode: dst(f, s), no LDS
        Td* dst = reinterpret_cast<Td*>(dst_base + op.dst) + int64_t(s0) * ldd + f0;
        dstrip y[HPL];  // beta != 0: every old value is requested before the first store
#pragma unroll
        for (int k = 0; k < HPL; ++k) {
            const int s = c0 + k * HCPP;
            y[k] = dstrip{};
            if (kind == COSTA_SCALE_AXPBY && (FULL || (nf_lane > 0 && s < ts)))
                y[k] = PR::load_dst(dst + s * ldd + lf, nf_lane, vd);
        }
#pragma unroll
        for (int k = 0; k < HPL; ++k) {
            const int s = c0 + k * HCPP;
            if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
            PR::store_dst(dst + s * ldd + lf, PR::compute(x[k], y[k], kind, alpha, beta), nf_lane, vd);
        }
        return;
    }

    // ---- transpose mode: dst(s, f) through LDS, staged in H
    Td* dst = reinterpret_cast<Td*>(dst_base + op.dst) + int64_t(f0) * ldd + s0;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    // store unit k of this lane: 64 s values of one f slot; after the lane exchange lane
    // (base + j) stores f = q*4 + j for s = sc*64 + base .. + 3
    auto unit = [&](int k, int& f, int& sb, int& n) {
        const int u = wave + HNW * k;
        const int sc = u / HQG, q = u % HQG;
        const int j = lane & (HV - 1);
        f = q * HV + j;
        sb = sc * HSW + (lane - j);
        n = FULL ? HV : ts - sb;
        return FULL || (f < tf && n > 0);
    };
    // beta != 0: the old destination values are requested now, with the source loads in flight
    dstrip old[HPS];
#pragma unroll
    for (int k = 0; k < HPS; ++k) {
        int f, sb, n;
        old[k] = dstrip{};
        if (kind == COSTA_SCALE_AXPBY && unit(k, f, sb, n)) old[k] = PR::load_dst(dst + f * ldd + sb, n, vd);
    }
#pragma unroll
    for (int k = 0; k < HPL; ++k) {
        const int s = c0 + k * HCPP;
        if (FULL || (nf_lane > 0 && s < ts)) {  // partial strips: the tail is 0, never stored
            u32x2h r;
            __builtin_memcpy(&r, &x[k], 8);
            *reinterpret_cast<u32x2h*>(tile + s * HP + lf) = r;
        }
    }
    __syncthreads();

    hstrip y[HPS];
#pragma unroll
    for (int k = 0; k < HPS; ++k) {
        const int u = wave + HNW * k;
        const int sc = u / HQG, q = u % HQG;
        const int s = sc * HSW + lane;
        y[k] = hstrip{{0, 0, 0, 0}};
        if (FULL || (s < ts && q * HV < tf)) {
            const u32x2h r = *reinterpret_cast<const u32x2h*>(tile + s * HP + q * HV);
            __builtin_memcpy(&y[k], &r, 8);
        }
    }
#pragma unroll
    for (int k = 0; k < HPS; ++k) {
        // the 4 x 4 block of 4 lanes, one element per 32-bit register (every lane takes part)
        vec<uint32_t> in;
#pragma unroll
        for (int e = 0; e < HV; ++e) in.e[e] = y[k].e[e];
        const vec<uint32_t> tr = lane_transpose(in, lane);
        int f, sb, n;
        if (!unit(k, f, sb, n)) continue;
        hstrip t;
#pragma unroll
        for (int e = 0; e < HV; ++e) t.e[e] = uint16_t(tr.e[e]);
        PR::store_dst(dst + f * ldd + sb, PR::compute(t, old[k], kind, alpha, beta), n, vd);
    }
}

template <typename H, bool SRC_F, bool DST_F>
__global__ __launch_bounds__(HNT) void half_kernel(const costa_tile_op_t* __restrict__ ops,
                                                   const uint64_t* __restrict__ work,
                                                   const char* src_base, char* dst_base,
                                                   const float* __restrict__ scalars) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* tile = reinterpret_cast<uint16_t*>(smem);
    // which sub-tile of which op (wave-uniform: scalar loads)
    const uint64_t w = work[blockIdx.x];
    const costa_tile_op_t op = ops[w >> 32];
    const uint32_t sub = uint32_t(w);
    const int nbf = (op.nf + HBF - 1) / HBF;
    const int f0 = int(sub % uint32_t(nbf)) * HBF;
    const int s0 = int(sub / uint32_t(nbf)) * HBS;
    const int tf = min(HBF, op.nf - f0);
    const int ts = min(HBS, op.ns - s0);
    const uint32_t slot = op.flags >> COSTA_SLOT_SHIFT;
    const float alpha = scalars[2 * slot];
    const float beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (tf == HBF && ts == HBS && (op.flags & vec_both) == vec_both)
        run_half<H, SRC_F, DST_F, true>(op, f0, s0, tf, ts, src_base, dst_base, alpha, beta, tile);
    else
        run_half<H, SRC_F, DST_F, false>(op, f0, s0, tf, ts, src_base, dst_base, alpha, beta, tile);
}

template <typename H, bool SRC_F, bool DST_F>
void launch_hpair(const costa_tile_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
                  const char* src_base, char* dst_base, const void* d_scalars, hipStream_t stream) {
    launch_strip<&half_kernel<H, SRC_F, DST_F>, kHalfLds>("half", HNT, l, stream, d_ops, d_work, src_base, dst_base,
                                                          static_cast<const float*>(d_scalars));
}

template <typename H>
void launch_h(bool src_f, bool dst_f, const costa_tile_op_t* d_ops, const uint64_t* d_work,
              const strip_list& l, const char* src_base, char* dst_base, const void* d_scalars,
              hipStream_t s) {
    if (src_f) launch_hpair<H, true, false>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else if (dst_f) launch_hpair<H, false, true>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else launch_hpair<H, false, false>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
}

void half_subtile(costa_dtype_t, costa_dtype_t, int* bf, int* bs) {
    *bf = HBF;
    *bs = HBS;
}

void launch_half(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* d_ops,
                 const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                 const void* d_scalars, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool src_f = src_dtype == COSTA_FLOAT, dst_f = dst_dtype == COSTA_FLOAT;
    const costa_dtype_t h = src_f ? dst_dtype : src_dtype;
    if (h == COSTA_HALF) launch_h<f16_t>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else launch_h<bf16_t>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, s);
}

}  // namespace

// (reached through the pair table of engine.cpp: half_pair(src, dst) holds)
pair_family half_family() { return {half_pair, half_subtile, launch_half}; }

}  // namespace engine
}  // namespace costa
