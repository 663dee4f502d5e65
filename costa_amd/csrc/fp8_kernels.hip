// FP8 tile kernels for CDNA4 (gfx950): the tile ops of transforms whose A or C holds a 1-byte
// element type Q (OCP e4m3fn or e5m2, raw bits),
//   Q -> Q (one Q), FLOAT -> Q, Q -> FLOAT      (costa_hip.h, "FP8").
// With w() the exact widening to fp32, cvt() the conversion fp32 -> Q (round to nearest even,
// subnormals kept; e4m3: above 448 -> NaN, e5m2: above 57344 -> +-inf) and g() tile_kernel's
// scale<float> (same branches, contraction off), an op computes, for its source element x and old
// destination value y,
//   Q -> Q        cvt(g(w(x), w(y)))         scale kind BITCOPY: the bits of x (a byte copy)
//   FLOAT -> Q    cvt(g(x, w(y)))            x is NOT rounded before the arithmetic
//   Q -> FLOAT    g(w(x), y)
// in copy mode dst(f, s), in transpose mode dst(s, f): fp32 arithmetic, one rounding at the store.
//
// One kernel family, fp8_kernel<Q, SRC_F, DST_F>, driven exactly like half_kernel by a
// costa_tile_op_t array and (op << 32) | sub-tile work items; one workgroup of 1024 threads runs
// one 128 x 128 sub-tile.  A lane's unit of work is a strip of 4 elements along the source's fast
// dimension: one dword on a Q side, 16 bytes on an fp32 side, so consecutive lanes touch
// consecutive addresses on both sides.
//   copy mode       no LDS: load strips, compute, store strips.  Whole Q -> Q sub-tiles take strips
//                   of 16 elements instead (16-byte accesses on both sides, one pass).
//   transpose mode  Q sources: the sub-tile is staged in LDS as Q bytes, rows s, pitch 128 + 4 bytes
//                   (33 dwords: one dword -- the access width -- of pad).  A half-wave then owns
//                   one quad of f for all 128 s: lane l reads the dwords of rows 4l .. 4l + 3 in an
//                   order rotated by l / 8 (rows 4 apart sit 4 banks apart, so without the rotation
//                   lanes l, l + 8, l + 16, l + 24 would share a bank), un-rotates them with
//                   selects, and transposes the 4 x 4 bytes inside the lane with v_perm_b32: four
//                   dwords of 4 consecutive s each.  Q targets add lane_transpose (DPP) over 4
//                   lanes, so every lane stores 16 consecutive s of one f (16 bytes); FLOAT targets
//                   widen each dword to a 16-byte store.
//                   FLOAT sources cannot be staged in Q (they are not rounded before the
//                   arithmetic): they are staged in fp32, pitch 128 + 4 elements, and go through
//                   half_kernel's scheme (ds_read_b128 of one strip, lane_transpose, one dword of
//                   4 consecutive s stored per lane).
// LDS: 128 x 132 = 16896 bytes (Q sources), 128 x 132 x 4 = 67584 bytes (FLOAT sources); none for
// copy-only lists.  No scratch.  Old destination values (beta != 0) are requested before the first
// wait.  Whole sub-tiles with both VEC flags take the FULL path, where every guard folds away;
// sub-tile remainders, ops below one strip and sides off their alignment (VEC flag clear) take
// the guarded, element-wise form of the same loads and stores: same values.
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

constexpr int QNT = 1024, QBF = 128, QBS = 128;  // threads, sub-tile (source fast x slow)
constexpr int QV = 4;                            // elements of a strip
constexpr int QLPC = QBF / QV;                   // lanes per source column (load)
constexpr int QCPP = QNT / QLPC;                 // source columns per load pass
constexpr int QPL = QBS / QCPP;                  // load passes
constexpr int QNW = QNT / 64;                    // wavefronts
constexpr int QPB = QBF + 4;                     // LDS row pitch of a Q tile (bytes)
constexpr int QPF = QBF + QV;                    // LDS row pitch of an fp32 tile (elements)
// Q tile: one half-wave per quad of f, 32 lanes x 4 s
static_assert(QBF / 4 == 2 * QNW && QBS == 32 * 4, "one store pass over a staged Q tile");
// fp32 tile (half_kernel's mapping): store unit = 64 s x one f slot
constexpr int QSW = 64;
constexpr int QQG = QBF / QV;
constexpr int QUNITS = (QBS / QSW) * QQG;
constexpr int QPS = QUNITS / QNW;
static_assert(QNT % QLPC == 0 && QBS % QCPP == 0 && QBS % QSW == 0 && QUNITS % QNW == 0, "mapping");
// whole Q -> Q copies: strips of 16 elements, every column in one pass
constexpr int QWV = 16;
static_assert((QBF / QWV) * QBS == QNT, "one pass of 16-byte strips");
constexpr size_t kFp8LdsQ = size_t(QBS) * QPB;
constexpr size_t kFp8LdsF = size_t(QBS) * QPF * 4;

// (e4m3_t / e5m2_t, the two 1-byte types, and round_finite: tile_device.hpp)
// a strip of 4 elements: of Q (one dword, element e in byte e) / of fp32 (16 bytes)
struct fstrip {
    float e[QV];
};
__device__ __forceinline__ uint32_t byte_of(uint32_t w, int e) { return (w >> (8 * e)) & 0xFFu; }

// one vector access where `vec_ok` (the side is aligned to the strip) and the strip is whole, else
// element by element; elements past n stay 0
__device__ __forceinline__ uint32_t load_q(const uint8_t* p, int n, bool vec_ok) {
    if (vec_ok && n >= QV) return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < QV; ++k)
        if (k < n) out |= uint32_t(p[k]) << (8 * k);
    return out;
}
__device__ __forceinline__ fstrip load_f(const float* p, int n, bool vec_ok) {
    fstrip out = {{0.f, 0.f, 0.f, 0.f}};
    if (vec_ok && n >= QV) {
        const raw16 r = ld16(p);
        __builtin_memcpy(&out, &r, 16);
    } else {
#pragma unroll
        for (int k = 0; k < QV; ++k)
            if (k < n) out.e[k] = p[k];
    }
    return out;
}
__device__ __forceinline__ void store_q(uint8_t* p, uint32_t in, int n, bool vec_ok) {
    if (vec_ok && n >= QV) {
        __builtin_nontemporal_store(in, reinterpret_cast<uint32_t*>(p));
    } else {
#pragma unroll
        for (int k = 0; k < QV; ++k)
            if (k < n) p[k] = uint8_t(byte_of(in, k));
    }
}
__device__ __forceinline__ void store_f(float* p, const fstrip& in, int n, bool vec_ok) {
    if (vec_ok && n >= QV) {
        raw16 r;
        __builtin_memcpy(&r, &in, 16);
        st16<true>(p, r);
    } else {
#pragma unroll
        for (int k = 0; k < QV; ++k)
            if (k < n) p[k] = in.e[k];
    }
}

// The pair's element types and the per-strip steps.  SRC_F / DST_F: that side holds fp32.
template <typename Q, bool SRC_F, bool DST_F>
struct qpair {
    using Ts = typename std::conditional<SRC_F, float, uint8_t>::type;
    using Td = typename std::conditional<DST_F, float, uint8_t>::type;
    using sstrip = typename std::conditional<SRC_F, fstrip, uint32_t>::type;
    using dstrip = typename std::conditional<DST_F, fstrip, uint32_t>::type;
    static_assert(!(SRC_F && DST_F), "one side at least holds the 1-byte type");

    static __device__ __forceinline__ sstrip load_src(const Ts* p, int n, bool vec_ok) {
        if constexpr (SRC_F) return load_f(p, n, vec_ok);
        else return load_q(p, n, vec_ok);
    }
    static __device__ __forceinline__ dstrip load_dst(const Td* p, int n, bool vec_ok) {
        if constexpr (DST_F) return load_f(p, n, vec_ok);
        else return load_q(p, n, vec_ok);
    }
    static __device__ __forceinline__ void store_dst(Td* p, const dstrip& o, int n, bool vec_ok) {
        if constexpr (DST_F) store_f(p, o, n, vec_ok);
        else store_q(p, o, n, vec_ok);
    }
    // 4 elements: x the source strip, y the old destination values (read only for AXPBY)
    static __device__ __forceinline__ dstrip compute(const sstrip& x, const dstrip& y, uint32_t kind,
                                                     float alpha, float beta) {
        if constexpr (!SRC_F && !DST_F) {
            if (kind == COSTA_SCALE_BITCOPY) return x;  // a byte copy: NaN payloads survive
        }
        dstrip o{};
#pragma unroll
        for (int e = 0; e < QV; ++e) {
            float xs, ys;
            if constexpr (SRC_F) xs = x.e[e];
            else xs = Q::widen(byte_of(x, e));
            if constexpr (DST_F) ys = y.e[e];
            else ys = Q::widen(byte_of(y, e));
            const float r = scale<float>(xs, ys, kind, false, alpha, beta);
            if constexpr (DST_F) o.e[e] = r;
            else o |= Q::narrow(r) << (8 * e);
        }
        return o;
    }
};

// the 4 x 4 byte transpose inside a lane: r[j] = row j (byte c = column c) -> t[c] = column c
// (byte j = row j).  v_perm_b32 picks each result byte from the 8 bytes {first : second operand}.
__device__ __forceinline__ void byte_transpose(const uint32_t r[4], uint32_t t[4]) {
    const uint32_t lo01 = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u);  // r0b0 r1b0 r0b1 r1b1
    const uint32_t hi01 = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);  // r0b2 r1b2 r0b3 r1b3
    const uint32_t lo23 = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u);
    const uint32_t hi23 = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
    t[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    t[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    t[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    t[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// A whole Q -> Q sub-tile in copy mode, both sides 16-byte aligned: strips of 16 elements.
template <typename Q>
__device__ __forceinline__ void run_qq_copy_full(const costa_tile_op_t& op, int f0, int s0,
                                                 const char* src_base, char* dst_base, float alpha,
                                                 float beta) {
    using PR = qpair<Q, false, false>;
    const uint32_t kind = (op.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const int lf = (int(threadIdx.x) % (QBF / QWV)) * QWV;
    const int s = int(threadIdx.x) / (QBF / QWV);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(src_base + op.src) + int64_t(s0 + s) * op.lds + f0 + lf;
    uint8_t* dst = reinterpret_cast<uint8_t*>(dst_base + op.dst) + int64_t(s0 + s) * op.ldd + f0 + lf;
    const raw16 x = ld16(src);
    raw16 y = {{0, 0, 0, 0}};
    if (kind == COSTA_SCALE_AXPBY) y = ld16(dst);
    raw16 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.w[k] = PR::compute(x.w[k], y.w[k], kind, alpha, beta);
    st16<true>(dst, o);
}

// One sub-tile.  FULL: a whole 128 x 128 sub-tile with both VEC flags, every guard folds away.
template <typename Q, bool SRC_F, bool DST_F, bool FULL>
__device__ __forceinline__ void run_fp8(const costa_tile_op_t& op, int f0, int s0, int tf_, int ts_,
                                        const char* src_base, char* dst_base, float alpha, float beta,
                                        unsigned char* tile) {
    using PR = qpair<Q, SRC_F, DST_F>;
    using Ts = typename PR::Ts;
    using Td = typename PR::Td;
    using sstrip = typename PR::sstrip;
    using dstrip = typename PR::dstrip;
    const int tf = FULL ? QBF : tf_;
    const int ts = FULL ? QBS : ts_;
    const uint32_t flags = op.flags;
    const uint32_t kind = (flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT;
    const bool vs = FULL || (flags & COSTA_TILE_VEC_SRC);
    const bool vd = FULL || (flags & COSTA_TILE_VEC_DST);
    const int64_t lds = op.lds, ldd = op.ldd;
    if constexpr (FULL && !SRC_F && !DST_F) {
        if (!(flags & COSTA_TILE_TRANSPOSE)) return run_qq_copy_full<Q>(op, f0, s0, src_base, dst_base, alpha, beta);
    }
    const Ts* src = reinterpret_cast<const Ts*>(src_base + op.src) + int64_t(s0) * lds + f0;

    // ---- load phase: lane -> (strip along f, column s); all loads issued first
    const int lf = (int(threadIdx.x) % QLPC) * QV;
    const int c0 = int(threadIdx.x) / QLPC;
    const int nf_lane = FULL ? QV : tf - lf;  // elements of this lane's strip inside the sub-tile
    sstrip x[QPL];
#pragma unroll
    for (int k = 0; k < QPL; ++k) {
        const int s = c0 + k * QCPP;
        x[k] = sstrip{};
        if (FULL || (nf_lane > 0 && s < ts)) x[k] = PR::load_src(src + s * lds + lf, nf_lane, vs);
    }

    if (!(flags & COSTA_TILE_TRANSPOSE)) {
        // ---- copy mode: dst(f, s), no LDS
        Td* dst = reinterpret_cast<Td*>(dst_base + op.dst) + int64_t(s0) * ldd + f0;
        dstrip y[QPL];  // beta != 0: every old value is requested before the first store
#pragma unroll
        for (int k = 0; k < QPL; ++k) {
            const int s = c0 + k * QCPP;
            y[k] = dstrip{};
            if (kind == COSTA_SCALE_AXPBY && (FULL || (nf_lane > 0 && s < ts)))
                y[k] = PR::load_dst(dst + s * ldd + lf, nf_lane, vd);
        }
#pragma unroll
        for (int k = 0; k < QPL; ++k) {
            const int s = c0 + k * QCPP;
            if (!FULL && (nf_lane <= 0 || s >= ts)) continue;
            PR::store_dst(dst + s * ldd + lf, PR::compute(x[k], y[k], kind, alpha, beta), nf_lane, vd);
        }
        return;
    }

    // ---- transpose mode: dst(s, f) through LDS
    Td* dst = reinterpret_cast<Td*>(dst_base + op.dst) + int64_t(f0) * ldd + s0;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;

    if constexpr (SRC_F) {
        // FLOAT -> Q: staged in fp32 (half_kernel's scheme).  Store unit k of this lane: 64 s values
        // of one f slot; after the lane exchange lane (base + j) stores f = q*4 + j for
        // s = sc*64 + base .. + 3
        float* ft = reinterpret_cast<float*>(tile);
        auto unit = [&](int k, int& f, int& sb, int& n) {
            const int u = wave + QNW * k;
            const int sc = u / QQG, q = u % QQG;
            const int j = lane & (QV - 1);
            f = q * QV + j;
            sb = sc * QSW + (lane - j);
            n = FULL ? QV : ts - sb;
            return FULL || (f < tf && n > 0);
        };
        // beta != 0: the old destination values are requested now, with the source loads in flight
        dstrip old[QPS];
#pragma unroll
        for (int k = 0; k < QPS; ++k) {
            int f, sb, n;
            old[k] = dstrip{};
            if (kind == COSTA_SCALE_AXPBY && unit(k, f, sb, n)) old[k] = PR::load_dst(dst + f * ldd + sb, n, vd);
        }
#pragma unroll
        for (int k = 0; k < QPL; ++k) {
            const int s = c0 + k * QCPP;
            if (FULL || (nf_lane > 0 && s < ts)) {  // partial strips: the tail is 0, never stored
                raw16 r;
                __builtin_memcpy(&r, &x[k], 16);
                *reinterpret_cast<raw16*>(ft + s * QPF + lf) = r;
            }
        }
        __syncthreads();
        vec<float> y[QPS];
#pragma unroll
        for (int k = 0; k < QPS; ++k) {
            const int u = wave + QNW * k;
            const int sc = u / QQG, q = u % QQG;
            const int s = sc * QSW + lane;
            y[k] = vec<float>{{0.f, 0.f, 0.f, 0.f}};
            if (FULL || (s < ts && q * QV < tf)) {
                const raw16 r = *reinterpret_cast<const raw16*>(ft + s * QPF + q * QV);
                __builtin_memcpy(&y[k], &r, 16);
            }
        }
#pragma unroll
        for (int k = 0; k < QPS; ++k) {
            const vec<float> tr = lane_transpose(y[k], lane);  // (every lane takes part)
            int f, sb, n;
            if (!unit(k, f, sb, n)) continue;
            sstrip t;
#pragma unroll
            for (int e = 0; e < QV; ++e) t.e[e] = tr.e[e];
            PR::store_dst(dst + f * ldd + sb, PR::compute(t, old[k], kind, alpha, beta), n, vd);
        }
    } else {
        // Q sources: staged as bytes.  This lane's block: f = 4q .. 4q + 3, s = 4l .. 4l + 3
        const int l = lane & 31, q = wave * 2 + (lane >> 5);
        const int fq = q * 4, sq = l * 4;
        // Q targets: after the exchange of 4 lanes, lane 4g + j stores f = 4q + j, s = 16g .. + 15
        const int j = l & 3, sg = (l - j) * 4;
        // beta != 0: the old destination values are requested now, with the source loads in flight
        raw16 old[DST_F ? 4 : 1];
#pragma unroll
        for (int c = 0; c < (DST_F ? 4 : 1); ++c) old[c] = raw16{{0, 0, 0, 0}};
        if (kind == COSTA_SCALE_AXPBY) {
            if constexpr (DST_F) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (FULL || (fq + c < tf && sq < ts)) {
                        const fstrip o = load_f(dst + (fq + c) * ldd + sq, FULL ? QV : ts - sq, vd);
                        __builtin_memcpy(&old[c], &o, 16);
                    }
            } else {
                if (FULL) {
                    old[0] = ld16(dst + (fq + j) * ldd + sg);
                } else if (fq + j < tf) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (sg + 4 * e < ts) old[0].w[e] = load_q(dst + (fq + j) * ldd + sg + 4 * e, ts - (sg + 4 * e), vd);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < QPL; ++k) {
            const int s = c0 + k * QCPP;
            if (FULL || (nf_lane > 0 && s < ts))  // partial strips: the tail is 0, never stored
                *reinterpret_cast<uint32_t*>(tile + s * QPB + lf) = x[k];
        }
        __syncthreads();
        // rows 4l .. 4l + 3 of this quad of f, read in an order rotated by l / 8 (conflict-free)
        const int rot = (l >> 3) & 3;
        uint32_t d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            d[i] = *reinterpret_cast<const uint32_t*>(tile + (sq + ((i + rot) & 3)) * QPB + fq);
        // d[i] holds row (i + rot) & 3: row jj is d[(jj - rot) & 3]
        uint32_t r[4], t[4];
        r[0] = sel4(rot, d[0], d[3], d[2], d[1]);
        r[1] = sel4(rot, d[1], d[0], d[3], d[2]);
        r[2] = sel4(rot, d[2], d[1], d[0], d[3]);
        r[3] = sel4(rot, d[3], d[2], d[1], d[0]);
        byte_transpose(r, t);  // t[c]: f = 4q + c, bytes = s 4l .. 4l + 3
        if constexpr (DST_F) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!FULL && (fq + c >= tf || sq >= ts)) continue;
                fstrip y;
                __builtin_memcpy(&y, &old[c], 16);
                store_f(dst + (fq + c) * ldd + sq, PR::compute(t[c], y, kind, alpha, beta), FULL ? QV : ts - sq, vd);
            }
        } else {
            vec<uint32_t> in;
#pragma unroll
            for (int c = 0; c < 4; ++c) in.e[c] = t[c];
            const vec<uint32_t> tr = lane_transpose(in, lane);  // (every lane takes part)
            raw16 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o.w[e] = PR::compute(tr.e[e], old[0].w[e], kind, alpha, beta);
            if (FULL) {
                st16<true>(dst + (fq + j) * ldd + sg, o);
            } else if (fq + j < tf) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (sg + 4 * e < ts) store_q(dst + (fq + j) * ldd + sg + 4 * e, o.w[e], ts - (sg + 4 * e), vd);
            }
        }
    }
}

template <typename Q, bool SRC_F, bool DST_F>
__global__ __launch_bounds__(QNT) void fp8_kernel(const costa_tile_op_t* __restrict__ ops,
                                                  const uint64_t* __restrict__ work,
                                                  const char* src_base, char* dst_base,
                                                  const float* __restrict__ scalars) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // which sub-tile of which op (wave-uniform: scalar loads)
    const uint64_t w = work[blockIdx.x];
    const costa_tile_op_t op = ops[w >> 32];
    const uint32_t sub = uint32_t(w);
    const int nbf = (op.nf + QBF - 1) / QBF;
    const int f0 = int(sub % uint32_t(nbf)) * QBF;
    const int s0 = int(sub / uint32_t(nbf)) * QBS;
    const int tf = min(QBF, op.nf - f0);
    const int ts = min(QBS, op.ns - s0);
    const uint32_t slot = op.flags >> COSTA_SLOT_SHIFT;
    const float alpha = scalars[2 * slot];
    const float beta = scalars[2 * slot + 1];
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    if (tf == QBF && ts == QBS && (op.flags & vec_both) == vec_both)
        run_fp8<Q, SRC_F, DST_F, true>(op, f0, s0, tf, ts, src_base, dst_base, alpha, beta, smem);
    else
        run_fp8<Q, SRC_F, DST_F, false>(op, f0, s0, tf, ts, src_base, dst_base, alpha, beta, smem);
}

template <typename Q, bool SRC_F, bool DST_F>
void launch_qpair(const costa_tile_op_t* d_ops, const uint64_t* d_work, const strip_list& l,
                  const char* src_base, char* dst_base, const void* d_scalars, hipStream_t stream) {
    // (the fp32 tile is over the default dynamic-LDS limit)
    launch_strip<&fp8_kernel<Q, SRC_F, DST_F>, (SRC_F ? kFp8LdsF : kFp8LdsQ)>(
        "fp8", QNT, l, stream, d_ops, d_work, src_base, dst_base, static_cast<const float*>(d_scalars));
}

template <typename Q>
void launch_q(bool src_f, bool dst_f, const costa_tile_op_t* d_ops, const uint64_t* d_work,
              const strip_list& l, const char* src_base, char* dst_base, const void* d_scalars,
              hipStream_t s) {
    if (src_f) launch_qpair<Q, true, false>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else if (dst_f) launch_qpair<Q, false, true>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else launch_qpair<Q, false, false>(d_ops, d_work, l, src_base, dst_base, d_scalars, s);
}

void fp8_subtile(costa_dtype_t, costa_dtype_t, int* bf, int* bs) {
    *bf = QBF;
    *bs = QBS;
}

void launch_fp8(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* d_ops,
                const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                const void* d_scalars, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool src_f = src_dtype == COSTA_FLOAT, dst_f = dst_dtype == COSTA_FLOAT;
    const costa_dtype_t q = src_f ? dst_dtype : src_dtype;
    if (q == COSTA_FP8_E4M3) launch_q<e4m3_t>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, s);
    else launch_q<e5m2_t>(src_f, dst_f, d_ops, d_work, l, src_base, dst_base, d_scalars, s);
}

}  // namespace

// (reached through the pair table of engine.cpp: fp8_pair(src, dst) holds)
pair_family fp8_family() { return {fp8_pair, fp8_subtile, launch_fp8}; }

}  // namespace engine
}  // namespace costa
