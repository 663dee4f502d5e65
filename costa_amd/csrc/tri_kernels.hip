// Edge-tile kernels of triangular transforms for CDNA4 (gfx950): the tiles a mask's diagonal cuts,
//   C(i, j) = beta*C(i, j) + alpha*op(A)(i, j)  where keep(i, j),   C(i, j) untouched elsewhere.
// An op is a costa_tri_op_t: a costa_tile_op_t plus the diagonal in the op's own coordinates,
//   copy mode       dst(f, s) = g(src(f, s))     where s - f >= diag (or <= diag: COSTA_TRI_LE)
//   transpose mode  dst(s, f) = g(src(f, s))     where ...
// g is tile_kernel's scale<T> with the same branches, contraction off, so a kept element equals the
// ordinary op's bit for bit.  Destination bytes at dropped positions are neither read nor written;
// source values there may be loaded but take part in no arithmetic that reaches a kept element
// (every element is computed on its own, and the Annex G recovery looks at kept elements only).
//
// One kernel family, tri_kernel<T>, driven like convert_kernel by a device array of ops and work
// items (op << 32) | (sub-tile << 1) | whole; one workgroup of 256 threads runs one 64 x 64
// sub-tile.  The planner cuts edge tiles to at most kTriCut rows by fewer columns with the diagonal
// through them, so an op is a few sub-tiles across and most of its area lies within a few
// sub-tiles of the diagonal: a small sub-tile leaves more of them whole (unmasked path) or empty
// (not listed at all), and 256 threads give every lane at least one 16-byte vector per pass for
// every element size.  The host builder lists only sub-tiles holding a kept element and marks the
// ones whose elements are all kept (`whole`).
//   whole, full-size, both sides on the 16-byte grid: the unmasked form, 16-byte loads and stores;
//       transposes are staged in LDS (rows s, pitch BF + V: 16 bytes of pad) and V lanes exchange
//       their V x V block, so every lane stores 16 bytes along the destination's fast dimension
//   every other sub-tile: the same loads and stores, guarded: a destination vector whose elements
//       are all kept is stored whole, one the diagonal cuts element by element (kept ones only),
//       one without a kept element is neither loaded from C nor stored; ragged remainders and
//       sides off the 16-byte grid (VEC flag clear) go element by element with the same values
// LDS: 64 x (64 + V) elements = 17 KiB (4-byte types) to 65 KiB (c128); copy-only lists take none.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "engine.hpp"
#include "strip_launch.hpp"
#include "strip_work.hpp"
#include "tile_device.hpp"

#pragma clang fp contract(off)

namespace costa {
namespace engine {
namespace {

constexpr int kTriNT = 256, kTriBF = 64, kTriBS = 64;

// sub-tile geometry (the load and store mappings of tile_kernels.hip `shape`)
template <typename T>
struct tshape {
    static constexpr int NT = kTriNT, BF = kTriBF, BS = kTriBS;
    static constexpr int V = vec<T>::V;
    static constexpr int P = BF + V;              // LDS row pitch (16-byte pad)
    static constexpr int LPC = BF / V;            // lanes per source column (load)
    static constexpr int CPP = NT / LPC;          // source columns per load pass
    static constexpr int PL = BS / CPP;           // load passes
    static constexpr int NW = NT / 64;            // wavefronts
    static constexpr int SW = 64;                 // s values of one store unit
    static constexpr int QG = BF / V;             // f slots (store units) per s chunk
    static constexpr int UNITS = (BS / SW) * QG;  // store units: 64 s x one f slot
    static constexpr int PS = UNITS / NW;         // store passes
    static_assert(NT % LPC == 0 && BS % CPP == 0 && BS % SW == 0 && UNITS % NW == 0, "mapping");
    static_assert(PL <= 32 && PS <= 32, "redo masks");
    static constexpr size_t lds_bytes = size_t(BS) * P * sizeof(T);
};

__device__ __forceinline__ int clampi(int64_t x, int n) { return x < 0 ? 0 : x > n ? n : int(x); }

// elements [klo, khi) of an n-element vector (n <= V) are kept
template <typename T>
__device__ __forceinline__ void mload(vec<T>& out, const T* p, int klo, int khi, int n, bool vec_ok) {
    constexpr int V = vec<T>::V;
    if (vec_ok && n >= V && klo == 0 && khi >= V) {
        const raw16 r = ld16(p);
        __builtin_memcpy(&out, &r, 16);
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (e >= klo && e < khi) out.e[e] = p[e];
    }
}
template <typename T>
__device__ __forceinline__ void mstore(T* p, const vec<T>& in, int klo, int khi, int n, bool vec_ok) {
    constexpr int V = vec<T>::V;
    if (vec_ok && n >= V && klo == 0 && khi >= V) {
        raw16 r;
        __builtin_memcpy(&r, &in, 16);
        st16<true>(p, r);
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (e >= klo && e < khi) p[e] = in.e[e];
    }
}

// One sub-tile.  FULL: a whole BF x BS sub-tile with both VEC flags whose elements are all kept:
// every guard folds away.
template <typename T, bool FULL>
__device__ __forceinline__ void run_tri(const costa_tile_op_t& op, int diag, bool whole, int f0, int s0,
                                        int tf_, int ts_, const char* src_base, char* dst_base, T alpha,
                                        T beta, T* tile) {
    using S = tshape<T>;
    constexpr int V = S::V, P = S::P;
    const int tf = FULL ? S::BF : tf_;
    const int ts = FULL ? S::BS : ts_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool conj = flags & COSTA_TILE_CONJ;
    const bool le = flags & COSTA_TRI_LE;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const bool vd = FULL || (flags & COSTA_TILE_VEC_DST);
    const int64_t lds = op.lds, ldd = op.ldd;
    const T* src = reinterpret_cast<const T*>(src_base + op.src) + int64_t(s0) * lds + f0;

    // ---- load phase: lane -> (vector along f, column s); all loads issued first
    const int lf = (int(threadIdx.x) % S::LPC) * V;
    const int c0 = int(threadIdx.x) / S::LPC;
    auto col_of = [&](int k) { return c0 + k * S::CPP; };
    const int nf_lane = FULL ? V : tf - lf;  // elements of this lane's vector inside the sub-tile
    vec<T> x[S::PL];
#pragma unroll
    for (int k = 0; k < S::PL; ++k) {
        const int s = col_of(k);
        if (FULL || (nf_lane > 0 && s < ts)) vload(x[k], src + s * lds + lf, nf_lane, vs);
    }

    if (!(flags & COSTA_TILE_TRANSPOSE)) {
        // ---- copy mode: dst(f, s) = g(src(f, s)), no LDS; the vector of column s holds
        // f = F .. F + n - 1: kept where f <= s - diag (or f >= s - diag)
        T* dst = reinterpret_cast<T*>(dst_base + op.dst) + int64_t(s0) * ldd + f0;
        const int n = FULL ? V : min(V, nf_lane);
        auto kept = [&](int s, int& klo, int& khi) {
            klo = 0;
            khi = n;
            if (FULL || whole) return;
            const int64_t x0 = int64_t(s0 + s) - diag - (f0 + lf);  // s - diag - F
            if (le) klo = clampi(x0, n);
            else khi = clampi(x0 + 1, n);
        };
        vec<T> y[S::PL];  // beta != 0: every old value is requested before the first store
        if (kind == COSTA_SCALE_AXPBY) {
#pragma unroll
            for (int k = 0; k < S::PL; ++k) {
                const int s = col_of(k);
                if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
                int klo, khi;
                kept(s, klo, khi);
                if (khi > klo) mload(y[k], dst + s * ldd + lf, klo, khi, n, vd);
            }
        }
        uint32_t redo = 0;  // complex vectors left for the Annex G path (bit k: vector k)
#pragma unroll
        for (int k = 0; k < S::PL; ++k) {
            const int s = col_of(k);
            if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
            int klo, khi;
            kept(s, klo, khi);
            if (khi <= klo) continue;
            vec<T> o;
            bool bad = false;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                bool b = false;
                o.e[e] = scale_naive(x[k].e[e], kind == COSTA_SCALE_AXPBY ? y[k].e[e] : e_zero<T>(), kind,
                                     conj, alpha, beta, b);
                bad = bad | (b & (e >= klo) & (e < khi));
            }
            if (is_cpx<T>::value && bad) {
                redo |= 1u << k;
                continue;
            }
            mstore(dst + s * ldd + lf, o, klo, khi, n, vd);
        }
        if constexpr (is_cpx<T>::value) {
            // vectors whose naive products needed the recovery: source and (not yet written)
            // destination are read again and every kept element goes through scale()
            if (__builtin_expect(redo != 0, 0)) {
#pragma unroll 1
                for (int k = 0; k < S::PL; ++k) {
                    if (!((redo >> k) & 1u)) continue;
                    const int s = col_of(k);
                    int klo, khi;
                    kept(s, klo, khi);
                    const T* a = src + s * lds + lf;
                    T* d = dst + s * ldd + lf;
#pragma unroll 1
                    for (int e = klo; e < khi; ++e)
                        d[e] = scale(a[e], kind == COSTA_SCALE_AXPBY ? d[e] : e_zero<T>(), kind, conj,
                                     alpha, beta);
                }
            }
        }
        return;
    }

    // ---- transpose mode: dst(s, f) = g(src(f, s)) through LDS
    T* dst = reinterpret_cast<T*>(dst_base + op.dst) + int64_t(f0) * ldd + s0;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    constexpr int SW = S::SW, QG = S::QG;
    // store unit k of this lane: 64 s values of one f slot; after the lane exchange lane
    // (base + j) stores f = q*V + j for s = sc*SW + base .. + V-1: kept where s >= diag + f (or <=)
    auto unit = [&](int k, int& f, int& sb, int& n, int& klo, int& khi) {
        const int u = wave + S::NW * k;
        const int sc = u / QG, q = u % QG;
        const int j = lane & (V - 1);
        f = q * V + j;
        sb = sc * SW + (lane - j);
        n = FULL ? V : min(V, ts - sb);
        klo = 0;
        khi = n;
        if (FULL) return true;
        if (f >= tf || n <= 0) return false;
        if (!whole) {
            const int64_t x0 = int64_t(diag) + (f0 + f) - (s0 + sb);  // diag + F - SB
            if (le) khi = clampi(x0 + 1, n);
            else klo = clampi(x0, n);
        }
        return khi > klo;
    };
    // beta != 0: the old destination values are requested now, with the source loads in flight
    vec<T> old[S::PS];
    if (kind == COSTA_SCALE_AXPBY) {
#pragma unroll
        for (int k = 0; k < S::PS; ++k) {
            int f, sb, n, klo, khi;
            if (unit(k, f, sb, n, klo, khi)) mload(old[k], dst + f * ldd + sb, klo, khi, n, vd);
        }
    }
#pragma unroll
    for (int k = 0; k < S::PL; ++k) {
        const int s = col_of(k);
        if (FULL || (nf_lane > 0 && s < ts)) {  // partial vectors: the tail is junk, never stored
            raw16 r;
            __builtin_memcpy(&r, &x[k], 16);
            *reinterpret_cast<raw16*>(tile + s * P + lf) = r;
        }
    }
    __syncthreads();

    vec<T> y[S::PS];
#pragma unroll
    for (int k = 0; k < S::PS; ++k) {
        const int u = wave + S::NW * k;
        const int sc = u / QG, q = u % QG;
        const int s = sc * SW + lane;
        if (FULL || (s < ts && q * V < tf)) {
            const raw16 r = *reinterpret_cast<const raw16*>(tile + s * P + q * V);
            __builtin_memcpy(&y[k], &r, 16);
        }
    }
    uint32_t redo = 0;  // complex store units left for the Annex G path (bit k: unit k)
#pragma unroll
    for (int k = 0; k < S::PS; ++k) {
        const vec<T> t = lane_transpose(y[k], lane);  // (every lane takes part in the exchange)
        int f, sb, n, klo, khi;
        if (!unit(k, f, sb, n, klo, khi)) continue;
        vec<T> o;
        bool bad = false;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            bool b = false;
            o.e[e] = scale_naive(t.e[e], kind == COSTA_SCALE_AXPBY ? old[k].e[e] : e_zero<T>(), kind, conj,
                                 alpha, beta, b);
            bad = bad | (b & (e >= klo) & (e < khi));
        }
        if (is_cpx<T>::value && bad) {
            redo |= 1u << k;
            continue;
        }
        mstore(dst + f * ldd + sb, o, klo, khi, n, vd);
    }
    if constexpr (is_cpx<T>::value) {
        // units whose naive products needed the recovery: element e of the unit is source row
        // sb + e, column f of the staged tile; its old value is still in the destination
        if (__builtin_expect(redo != 0, 0)) {
#pragma unroll 1
            for (int k = 0; k < S::PS; ++k) {
                if (!((redo >> k) & 1u)) continue;
                int f, sb, n, klo, khi;
                unit(k, f, sb, n, klo, khi);
                T* d = dst + f * ldd + sb;
#pragma unroll 1
                for (int e = klo; e < khi; ++e)
                    d[e] = scale(tile[(sb + e) * P + f], kind == COSTA_SCALE_AXPBY ? d[e] : e_zero<T>(),
                                 kind, conj, alpha, beta);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kTriNT) void tri_kernel(const costa_tri_op_t* __restrict__ ops,
                                                     const uint64_t* __restrict__ work,
                                                     const char* src_base, char* dst_base,
                                                     const T* __restrict__ scalars) {
    using S = tshape<T>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* tile = reinterpret_cast<T*>(smem);
    // which sub-tile of which op (wave-uniform: scalar loads)
    const uint64_t w = work[blockIdx.x];
    const costa_tri_op_t top = ops[w >> 32];
    const costa_tile_op_t& op = top.op;
    const uint32_t sub = uint32_t(w) >> 1;
    const bool whole = w & 1u;
    const int nbf = (op.nf + S::BF - 1) / S::BF;
    const int f0 = int(sub % uint32_t(nbf)) * S::BF;
    const int s0 = int(sub / uint32_t(nbf)) * S::BS;
    const int tf = min(S::BF, op.nf - f0);
    const int ts = min(S::BS, op.ns - s0);
    const uint32_t slot = op.flags >> COSTA_SLOT_SHIFT;
    const T alpha = scalars[2 * slot];
    const T beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (whole && tf == S::BF && ts == S::BS && (op.flags & vec_both) == vec_both)
        run_tri<T, true>(op, top.diag, true, f0, s0, tf, ts, src_base, dst_base, alpha, beta, tile);
    else
        run_tri<T, false>(op, top.diag, whole, f0, s0, tf, ts, src_base, dst_base, alpha, beta, tile);
}

template <typename T>
void launch_type(const costa_tri_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
                 const char* src_base, char* dst_base, const void* d_scalars, hipStream_t stream) {
    using S = tshape<T>;
    // (c128's tile is over the default dynamic-LDS limit)
    launch_strip<&tri_kernel<T>, S::lds_bytes>("tri", S::NT, l, stream, d_ops, d_work, src_base, dst_base,
                                               static_cast<const T*>(d_scalars));
}

}  // namespace

void tri_subtile(costa_dtype_t dtype, int* bf, int* bs) {
    (void)dtype_size(dtype);  // (throws for an unknown dtype)
    *bf = kTriBF;
    *bs = kTriBS;
}

strip_list build_tri_work(costa_dtype_t dtype, const std::vector<costa_tri_op_t>& ops, uint64_t src_base,
                          uint64_t dst_base, std::vector<costa_tri_op_t>& ordered,
                          std::vector<uint64_t>& work) {
    const int64_t bf = kTriBF, bs = kTriBS;
    const uint64_t E = dtype_size(dtype);
    // a sub-tile is listed when s - f reaches the kept side of the diagonal somewhere in it, whole
    // when everywhere
    auto sub_of = [=](const costa_tri_op_t& t, int64_t i, int64_t j) {
        const bool le = t.op.flags & COSTA_TRI_LE;
        const int64_t d = t.diag;
        const int64_t f0 = i * bf, f1 = std::min<int64_t>(t.op.nf, f0 + bf) - 1;
        const int64_t s0 = j * bs, s1 = std::min<int64_t>(t.op.ns, s0 + bs) - 1;
        const int64_t v_min = s0 - f1, v_max = s1 - f0;
        if (le ? v_min > d : v_max < d) return strip_sub::skip;
        return (le ? v_max <= d : v_min >= d) ? strip_sub::whole : strip_sub::listed;
    };
    return build_strip_work<true>("edge-tile", ops, src_base, dst_base, kTriBF, kTriBS, E, E,
                                  strip_alignment(strip_family::tri, E, E), ordered, work, sub_of);
}

void launch_tri(costa_dtype_t dtype, const costa_tri_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
                const char* src_base, char* dst_base, const void* d_scalars, void* stream) {
    if (l.n_items <= 0) return;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
    case COSTA_FLOAT: launch_type<float>(d_ops, d_work, l, src_base, dst_base, d_scalars, s); break;
    case COSTA_DOUBLE: launch_type<double>(d_ops, d_work, l, src_base, dst_base, d_scalars, s); break;
    case COSTA_CFLOAT: launch_type<cpx<float>>(d_ops, d_work, l, src_base, dst_base, d_scalars, s); break;
    case COSTA_CDOUBLE: launch_type<cpx<double>>(d_ops, d_work, l, src_base, dst_base, d_scalars, s); break;
    case COSTA_INT32: launch_type<int>(d_ops, d_work, l, src_base, dst_base, d_scalars, s); break;
    default: throw error(COSTA_ERR_ARG, "unknown dtype");
    }
}

}  // namespace engine
}  // namespace costa
