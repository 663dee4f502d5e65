// Executor: device workspaces, plan cache, host staging, and the exchange.
//
// One transform = the reference's exchange_async (grid2grid/transform.cpp:46-128) re-laid
// for one GPU per rank:
//   main stream : [H2D of host-resident data] -> PACK kernel -> RCCL send/recv (all peers,
//                 one group) -> UNPACK kernel -> [D2H]
//   aux stream  : LOCAL kernel, overlapping pack + exchange (the reference overlaps its
//                 local copy with the MPI messages in flight, transform.cpp:96-101)
// Plans are cached by layout content (the reference re-plans every call).
#include <exception>
#include <thread>
#include "engine.hpp"
#include "strip_work.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <numeric>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <list>
#include <map>
#include <mutex>
#include <unordered_map>

namespace costa {
namespace engine {

#define HIP_CHECK(x)                                                                   \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess)                                                          \
            throw error(COSTA_ERR_HIP, std::string(#x " failed: ") + hipGetErrorString(e_)); \
    } while (0)
#define NCCL_CHECK(x)                                                                   \
    do {                                                                                \
        ncclResult_t r_ = (x);                                                          \
        if (r_ != ncclSuccess)                                                          \
            throw error(COSTA_ERR_NCCL, std::string(#x " failed: ") + ncclGetErrorString(r_)); \
    } while (0)

// ---------------------------------------------------------------- statistics
namespace {
costa_stats_t g_stats{};
bool g_profiling = false;
std::recursive_mutex g_mutex;  // transforms of one process are serialised (the reference's
                               // per-type workspace singleton is not re-entrant either)
}  // namespace
costa_stats_t& stats() { return g_stats; }
bool profiling() { return g_profiling; }
void set_profiling(bool on) { g_profiling = on; }

// ---------------------------------------------------------------- device memory
struct dbuf {
    void* p = nullptr;
    size_t n = 0;
    dbuf() = default;
    dbuf(const dbuf&) = delete;
    dbuf& operator=(const dbuf&) = delete;
    ~dbuf() {
        if (p) (void)hipFree(p);
    }
    void reserve(size_t bytes) {
        if (bytes <= n) return;
        if (p) HIP_CHECK(hipFree(p));
        p = nullptr;
        n = 0;
        // round up to 2 MiB so growing workspaces do not reallocate every call
        size_t want = (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
        HIP_CHECK(hipMalloc(&p, want));
        n = want;
    }
    template <typename X>
    void upload(const std::vector<X>& v, hipStream_t s) {
        if (v.empty()) return;
        reserve(v.size() * sizeof(X));
        HIP_CHECK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice, s));
    }
};

// ---------------------------------------------------------------- per-device context
struct device_ctx {
    struct timed {
        int phase;
        hipEvent_t a, b;
    };
    int device = 0;
    hipStream_t main = nullptr, aux = nullptr, xch = nullptr;  // xch: the RCCL exchange rounds
    hipEvent_t ev_ready = nullptr, ev_local = nullptr, ev_user = nullptr, ev_done = nullptr;
    std::vector<hipEvent_t> ev_packed, ev_moved;  // per exchange round
    void round_events(size_t n) {
        while (ev_packed.size() < n) {
            hipEvent_t a, b;
            HIP_CHECK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&b, hipEventDisableTiming));
            ev_packed.push_back(a);
            ev_moved.push_back(b);
        }
    }
    std::vector<hipEvent_t> free_events;  // timing events ready for reuse
    std::deque<timed> pending;            // recorded phase brackets not yet read
    dbuf send, recv;
    dbuf amax_ops, amax_work;  // the op and work lists of costa_hip_layout_amax calls
    explicit device_ctx(int dev) : device(dev) {
        HIP_CHECK(hipSetDevice(dev));
        // blocking streams: they order after work on the legacy default stream
        HIP_CHECK(hipStreamCreate(&main));
        HIP_CHECK(hipStreamCreate(&aux));
        HIP_CHECK(hipStreamCreate(&xch));
        for (hipEvent_t* e : {&ev_ready, &ev_local, &ev_user, &ev_done})
            HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    ~device_ctx() {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(main);
        (void)hipStreamSynchronize(aux);
        (void)hipStreamSynchronize(xch);
        for (auto e : ev_packed) (void)hipEventDestroy(e);
        for (auto e : ev_moved) (void)hipEventDestroy(e);
        for (auto& t : pending) {
            (void)hipEventDestroy(t.a);
            (void)hipEventDestroy(t.b);
        }
        for (auto e : free_events) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_ready, ev_local, ev_user, ev_done}) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(main);
        (void)hipStreamDestroy(aux);
        (void)hipStreamDestroy(xch);
    }
    hipEvent_t take_event();
    void resolve(size_t max_n = size_t(-1));  // read finished brackets into the statistics
};

namespace {
std::map<int, std::unique_ptr<device_ctx>>& ctx_map() {
    static std::map<int, std::unique_ptr<device_ctx>> m;
    return m;
}
device_ctx& ctx(int device) {
    auto& m = ctx_map();
    auto it = m.find(device);
    if (it == m.end()) it = m.emplace(device, std::make_unique<device_ctx>(device)).first;
    HIP_CHECK(hipSetDevice(device));
    return *it->second;
}
}  // namespace

// ---------------------------------------------------------------- communicator
struct comm {
    int rank = 0, size = 1, device = 0;
    ncclComm_t nccl = nullptr;
    // rank emulation (test mode, comm_emulated): planned like an RCCL communicator of `size` ranks;
    // a transform launches only the selected part (comm_emulate) against the caller's package
    bool emulated = false;
    int part = 0;   // 0 = none selected yet, else COSTA_EMULATE_PACK / _UNPACK / _LOCAL
    int round = -1; // of PACK / UNPACK: 0 .. exchange_rounds() - 1, or -1 = every round in order
    void* buffer = nullptr;  // the caller's send (PACK) / receive (UNPACK) package
    // whether its plans have exchange rounds and package lists
    bool exchanges() const { return nccl != nullptr || emulated; }
    ~comm() {
        if (nccl) (void)ncclCommDestroy(nccl);
    }
};

int device_count() {
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    return n;
}

int rccl_version() {
    int v = 0;
    NCCL_CHECK(ncclGetVersion(&v));
    return v;
}

namespace {
comm* new_comm(int device) {
    const int n = device_count();
    if (device < 0 || device >= n) throw error(COSTA_ERR_ARG, "costa: device index out of range");
    auto* c = new comm;
    c->device = device;
    return c;
}

void init_nccl(comm* c, const ncclUniqueId& uid, int nranks, int rank, const char* what) {
    HIP_CHECK(hipSetDevice(c->device));
    ncclResult_t r = ncclCommInitRank(&c->nccl, nranks, uid, rank);
    if (r != ncclSuccess) {
        delete c;
        throw error(COSTA_ERR_NCCL, std::string(what) + ": " + ncclGetErrorString(r));
    }
}
}  // namespace

comm* comm_self(int device) {
    comm* c = new_comm(device);
    if (loopback_exchange()) {  // test mode: a real one-rank RCCL communicator
        ncclUniqueId uid;
        NCCL_CHECK(ncclGetUniqueId(&uid));
        init_nccl(c, uid, 1, 0, "loopback ncclCommInitRank");
    }
    return c;
}

comm* comm_create(const unsigned char* id, int nranks, int rank, int device) {
    if (nranks < 1 || rank < 0 || rank >= nranks) throw error(COSTA_ERR_ARG, "costa: bad rank/size");
    if (nranks == 1) return comm_self(device);
    comm* c = new_comm(device);
    c->rank = rank;
    c->size = nranks;
    ncclUniqueId uid;
    std::memcpy(uid.internal, id, NCCL_UNIQUE_ID_BYTES);
    init_nccl(c, uid, nranks, rank, "ncclCommInitRank");
    return c;
}

namespace {
bool is_device_ptr(const void* p);
}

comm* comm_emulated(int rank, int nranks, int device) {
    if (nranks < 1 || rank < 0 || rank >= nranks) throw error(COSTA_ERR_ARG, "costa: bad rank/size");
    comm* c = new_comm(device);
    c->rank = rank;
    c->size = nranks;
    c->emulated = true;
    return c;
}

void comm_emulate(comm* c, int part, int round, void* buffer) {
    if (!c) throw error(COSTA_ERR_ARG, "costa: null communicator");
    if (!c->emulated)
        throw error(COSTA_ERR_ARG, "costa_hip_comm_emulate: not an emulated communicator "
                                   "(costa_hip_comm_emulated makes one)");
    if (part != COSTA_EMULATE_PACK && part != COSTA_EMULATE_UNPACK && part != COSTA_EMULATE_LOCAL)
        throw error(COSTA_ERR_ARG, "costa_hip_comm_emulate: part is not PACK, UNPACK or LOCAL");
    if (part == COSTA_EMULATE_LOCAL) {
        round = -1;
        buffer = nullptr;
    } else {
        if (round < -1 || round >= exchange_rounds())
            throw error(COSTA_ERR_ARG, "costa_hip_comm_emulate: round is not -1 or below "
                                       "costa_hip_exchange_rounds()");
        HIP_CHECK(hipSetDevice(c->device));
        if (!buffer || !is_device_ptr(buffer))
            throw error(COSTA_ERR_ARG, "costa_hip_comm_emulate: the package buffer is not a device pointer");
        if (reinterpret_cast<uintptr_t>(buffer) % 256)
            throw error(COSTA_ERR_ARG, "costa_hip_comm_emulate: the package buffer is not aligned to "
                                       "256 bytes");
    }
    c->part = part;
    c->round = round;
    c->buffer = buffer;
}

const char* tuning_env(const char* name) {
    static const bool on = [] {
        const char* s = std::getenv("COSTA_TUNING");
        return s && std::atoi(s) == 1;
    }();
    return on ? std::getenv(name) : nullptr;
}

int loopback_exchange() {
    static const int mode = [] {
        const char* s = std::getenv("COSTA_LOOPBACK");
        const int m = s ? std::atoi(s) : 0;
        return m == 1 || m == 2 ? m : 0;
    }();
    return mode;
}

// Largest ncclSend / ncclRecv: 256 MiB by default (override COSTA_MAX_MSG_BYTES), never more
// than kMaxMessageCap.  A single self send/recv above 2^30 bytes delivered only its first half
// (the failure starts where twice the byte count passes INT32_MAX, and the lost
// part is exactly the second of two halves); the last size measured intact was 2^30 - 233472
// bytes, so the cap stays 1 MiB below 2^30 (exactly 2^30 is already on the failing side of
// 2 * count > INT32_MAX).  tests/test_gpu_rccl_system.py moves a package in pieces of the cap.
constexpr size_t kMaxMessageCap = (size_t(1) << 30) - (size_t(1) << 20);
size_t max_message_bytes() {
    static const size_t v = [] {
        const char* s = std::getenv("COSTA_MAX_MSG_BYTES");  // tuning override
        const long long x = s ? std::atoll(s) : 0;
        const size_t want = x > 0 ? size_t(x) : (size_t(1) << 28);
        return std::min(want, kMaxMessageCap);
    }();
    return v;
}

// Exchange rounds: a peer's package of at least kRoundMinBytes moves in exchange_rounds() equal
// parts, each its own RCCL group on the exchange stream, so that packing part r+1, moving part
// r and unpacking part r-1 overlap.  Both sides of a pair derive the parts from the pair's
// element count alone, so they agree on every message.
constexpr size_t kRoundMinBytes = size_t(16) << 20;
int exchange_rounds() {
    static const int v = [] {
        const char* s = std::getenv("COSTA_EXCHANGE_ROUNDS");  // tuning / reproduction override
        const int x = s ? std::atoi(s) : 4;
        return std::max(1, std::min(16, x));
    }();
    return v;
}

// (COSTA_ROUND_MIN_BYTES, tuning: another threshold, so that the GPU tests have plans of several
// rounds at fixture size; every rank must agree)
size_t round_min_bytes() {
    static const size_t v = [] {
        const char* s = tuning_env("COSTA_ROUND_MIN_BYTES");
        const long long x = s ? std::atoll(s) : 0;
        return x > 0 ? size_t(x) : kRoundMinBytes;
    }();
    return v;
}

namespace {
int parts_of(int64_t n, size_t E, int R) { return size_t(n) * E >= round_min_bytes() ? R : 1; }
}  // namespace
// element range [lo, hi) of round r of a package of n elements (empty past its parts)
void round_range(int64_t n, size_t E, int R, int r, int64_t& lo, int64_t& hi) {
    const int parts = parts_of(n, E, R);
    if (r >= parts) {
        lo = hi = n;
        return;
    }
    lo = n * r / parts;
    hi = n * (r + 1) / parts;
}
namespace {
// round holding element o (0 <= o < n) of a package of n elements
int round_of(int64_t o, int64_t n, size_t E, int R) {
    const int parts = parts_of(n, E, R);
    int r = int(o * parts / n);
    while (r > 0 && o < n * r / parts) --r;
    while (r + 1 < parts && o >= n * (r + 1) / parts) ++r;
    return r;
}
// the peer whose package holds element o of a buffer laid out by displs / counts
size_t peer_of(const std::vector<int64_t>& displs, int64_t o) {
    const auto it = std::upper_bound(displs.begin(), displs.end(), o);
    return size_t(it - displs.begin()) - 1;
}
}  // namespace

namespace {
// The one round-assignment rule: the round of the op at byte `offset` of the send (pack) or receive
// (unpack) package that covers `units` package units.  A pack op goes by its first unit (everything a
// round sends is packed by then), an unpack op by its last (everything it reads has arrived); an op
// lies inside one peer's package.  (tools/work_check.cpp rounds)
int round_of_op(const plan& p, int rounds, bool unpack, uint64_t offset, int64_t units) {
    const size_t E = pkg_unit_size(p.pkg_dtype);  // package offsets are in package elements (units)
    const std::vector<int64_t>& displs = unpack ? p.recv_displs : p.send_displs;
    const std::vector<int64_t>& counts = unpack ? p.recv_counts : p.send_counts;
    const int64_t first = int64_t(offset / E);
    const size_t q = peer_of(displs, first);
    return round_of((unpack ? first + units - 1 : first) - displs[q], counts[q], E, rounds);
}
}  // namespace

void exchange_round_of_ops(const plan& p, int rounds, std::vector<int>& pack_round,
                           std::vector<int>& unpack_round) {
    pack_round.clear();
    unpack_round.clear();
    for (const auto& op : p.pack_ops) pack_round.push_back(round_of_op(p, rounds, false, op.dst, 1));
    for (const auto& op : p.unpack_ops)
        unpack_round.push_back(round_of_op(p, rounds, true, op.src, int64_t(op.nf) * op.ns));
}

void exchange_round_of_tri(const plan& p, int rounds, std::vector<int>& unpack_tri_round) {
    unpack_tri_round.clear();
    for (const auto& t : p.unpack_tri)
        unpack_tri_round.push_back(round_of_op(p, rounds, true, t.op.src, int64_t(t.op.nf) * t.op.ns));
}

void exchange_round_of_scaled(const plan& p, int rounds, std::vector<int>& unpack_round) {
    unpack_round.clear();
    for (const auto& t : p.unpack_scaled)  // (of a packed package: the bytes of its nf x ns elements)
        unpack_round.push_back(
            round_of_op(p, rounds, true, t.op.src, pkg_units(p.pkg_dtype, int64_t(t.op.nf) * t.op.ns)));
}

int comm_rank(const comm* c) { return c->rank; }
int comm_size(const comm* c) { return c->size; }
void comm_destroy(comm* c) { delete c; }

void comm_unique_id(unsigned char* out) {
    ncclUniqueId uid;
    NCCL_CHECK(ncclGetUniqueId(&uid));
    std::memcpy(out, uid.internal, NCCL_UNIQUE_ID_BYTES);
}

// ---------------------------------------------------------------- work lists
bool any_transpose(const std::vector<costa_tile_op_t>& ops) {
    for (const auto& op : ops)
        if (op.flags & COSTA_TILE_TRANSPOSE) return true;
    return false;
}

bool any_axpby(const std::vector<costa_tile_op_t>& ops) {
    for (const auto& op : ops)
        if (((op.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT) == COSTA_SCALE_AXPBY) return true;
    return false;
}

// Work classes.  An op goes to the large shape (a 1024-thread workgroup per sub-tile) when it
// holds at least half a large sub-tile of data; every other op runs on the wavefront path
// (tiny_kernel): ops over a wavefront's budget are first cut, here on the host, into
// rectangular sub-ops within it (a sub-rectangle of a tile op is a tile op).  Budgets: copy
// mode one wavefront pass of data (tiny_copy_budget), transpose mode tiny_lds_budget() of staged
// tile (row pitch nf | 1).
// Copy mode: a part of one wavefront pass (64 lanes x tiny_copy_lane_bytes), an op the wavefront
// moves in one round trip, cut finer for more wavefronts in flight.  Local lists: half (2 KiB);
// r3 with the XCD column bands, cfg 5 'N' 0.434-0.436 ms at 2 KiB against 0.446-0.447 at 3 KiB,
// 0.438 at 2.5, 0.449-0.451 at 1.5, 0.466 at 4, 0.517 at 1 (profiles/r3b/README.md §copy_budget).  Pack
// and unpack lists (one side the dense package): three quarters (3 KiB); through the loopback
// exchange pack 'N' 0.587-0.590 ms against 0.607-0.608 at 2 KiB, unpack 0.592-0.597 against
// 0.607-0.608 (profiles/r3b/README.md §copy_budget; r11: 3 KiB best for every list,
// profiles/r11/c5_budget_uc64.log).
// (COSTA_TINY_COPY: another budget in bytes up to kTinyCopyBytes, tuning runs only)
int64_t tiny_copy_budget(int64_t E, bool local) {
    static const int64_t env = [] {
        const char* s = tuning_env("COSTA_TINY_COPY");
        const int64_t v = s ? std::atoll(s) : 0;
        return v >= 256 && v <= kTinyCopyBytes ? v : int64_t(0);
    }();
    return env ? env : (local ? 32 : 48) * int64_t(tiny_copy_lane_bytes(size_t(E)));
}

// Transpose mode: the staged tile, kTinyLdsDefault bytes of LDS per wavefront
// (COSTA_TINY_LDS: another budget up to kTinyLdsBytes, tuning runs only)
int64_t tiny_lds_budget() {
    static const int64_t b = [] {
        const char* s = tuning_env("COSTA_TINY_LDS");
        const int64_t v = s ? std::atoll(s) : 0;
        return v >= 256 && v <= kTinyLdsBytes ? v : int64_t(kTinyLdsDefault);
    }();
    return b;
}

static bool is_tiny(const costa_tile_op_t& op, int64_t E, bool local) {
    // (elements against budget / E: nf * ns * E passes 2^63 for an op of 2^31 x 2^31, which then
    // looked tiny instead of being refused as too large)
    if (op.flags & COSTA_TILE_TRANSPOSE) return int64_t(op.nf | 1) * op.ns <= tiny_lds_budget() / E;
    return int64_t(op.nf) * op.ns <= tiny_copy_budget(E, local) / E;
}

static uint32_t vec_flags(uint64_t src, int64_t lds, uint64_t dst, int64_t ldd, int64_t E) {
    uint32_t f = 0;
    if (src % 16 == 0 && (lds * E) % 16 == 0) f |= COSTA_TILE_VEC_SRC;
    if (dst % 16 == 0 && (ldd * E) % 16 == 0) f |= COSTA_TILE_VEC_DST;
    return f;
}

// cut `op` into near-equal rectangles that each fit the wavefront budget: the grid of pieces
// (nfc x nsc pieces of cf x cs elements at most), then the pieces themselves
namespace {
struct wave_grid {
    int64_t nfc = 1, nsc = 1;
};
wave_grid wave_pieces(const costa_tile_op_t& op, int64_t E, bool local) {
    wave_grid g;
    if (is_tiny(op, E, local)) return g;
    const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
    const int64_t budget = (tr ? tiny_lds_budget() : tiny_copy_budget(E, local)) / E;  // elements
    const int64_t nf = op.nf, ns = op.ns;
    // transpose: pieces at most 16 elements wide along f (the source's contiguous dimension),
    // as tall along s as the budget allows: the destination runs (which a beta != 0 op both reads
    // and writes) stay long.  cfg 5 'T' 0.726 ms with near-square pieces (32 wide), 0.716 with 16,
    // 0.728 with 12, 0.758 with 8, 0.754 cut along s first; fp64 / c64 / c128 pack and unpack
    // lists equal at 16 (profiles/r3b/README.md §side).  Copy: whole columns when one fits, else tall pieces
    static const int64_t side_env = [] {  // COSTA_TR_SIDE (tuning): the cut's side along f
        const char* v = tuning_env("COSTA_TR_SIDE");
        return v ? std::max<int64_t>(1, std::atoll(v)) : int64_t(0);
    }();
    const int64_t sq_side = std::max<int64_t>(1, int64_t(std::sqrt(double(budget))));
    const int64_t side = tr ? (side_env ? side_env : std::min<int64_t>(16, sq_side)) : budget;
    g.nfc = (nf + side - 1) / side;
    const int64_t cf = (nf + g.nfc - 1) / g.nfc;
    const int64_t cs_max = std::max<int64_t>(1, budget / (tr ? (cf | 1) : cf));
    g.nsc = (ns + cs_max - 1) / cs_max;
    return g;
}
// writes the g.nfc * g.nsc pieces of `op` at `out`
void emit_pieces(const costa_tile_op_t& op, int64_t E, const wave_grid& g, bool local, costa_tile_op_t* out) {
    if (g.nfc == 1 && g.nsc == 1) {
        *out = op;
        return;
    }
    const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
    const int64_t nf = op.nf, ns = op.ns;
    const uint32_t keep = op.flags & ~uint32_t(COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST);
    for (int64_t i = 0; i < g.nfc; ++i) {
        const int64_t f0 = i * nf / g.nfc, f1 = (i + 1) * nf / g.nfc;
        for (int64_t j = 0; j < g.nsc; ++j) {
            const int64_t s0 = j * ns / g.nsc, s1 = (j + 1) * ns / g.nsc;
            costa_tile_op_t sub = op;
            sub.src = op.src + uint64_t((s0 * op.lds + f0) * E);
            sub.dst = op.dst + uint64_t((tr ? f0 * op.ldd + s0 : s0 * op.ldd + f0) * E);
            sub.nf = int32_t(f1 - f0);
            sub.ns = int32_t(s1 - s0);
            sub.flags = keep | vec_flags(sub.src, op.lds, sub.dst, op.ldd, E);
            if (!is_tiny(sub, E, local)) throw error(COSTA_ERR_INTERNAL, "costa: wave split over budget");
            *out++ = sub;
        }
    }
}

// XCD column bands (wave_knobs::xcd_bands): the tiny kernel gives XCD x the x-th eighth of
// the list; destination order alone makes that eighth a run of whole target block-rows, so an A
// cache line shared by the tiles above and below a block-row boundary is fetched again one
// block-row of the XCD's traffic later (~11 MB for cfg 5: past its 4 MB L2).  Here the list is
// first split into eight bands of target columns (by the planner's column-major hint, equal piece
// counts), each band in destination order: every XCD walks all block-rows of its own columns, and
// the two tiles sharing the line run ~1/8 of a block-row apart on the same XCD.
void xcd_bands(const std::vector<const costa_tile_op_t*>& ops, int64_t E, int k, bool local,
               std::vector<uint32_t>& perm) {
    const uint64_t nb = 8 * uint64_t(k);  // bands: XCD x walks bands k x .. k x + k - 1 in turn
    const size_t n = perm.size();
    std::vector<uint64_t> pieces(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const wave_grid g = wave_pieces(*ops[i], E, local);
        pieces[i] = uint64_t(g.nfc * g.nsc);
        total += pieces[i];
    }
    std::vector<uint32_t> by_hint(n);
    for (size_t i = 0; i < n; ++i) by_hint[i] = uint32_t(i);
    std::stable_sort(by_hint.begin(), by_hint.end(),
                     [&](uint32_t x, uint32_t y) { return ops[x]->order < ops[y]->order; });
    std::vector<uint32_t> band(n);
    uint64_t cum = 0;
    for (const uint32_t i : by_hint) {
        band[i] = uint32_t(std::min<uint64_t>(nb - 1, cum * nb / std::max<uint64_t>(total, 1)));
        cum += pieces[i];
    }
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return band[x] < band[y]; });
}

// (key, item) pairs whose items ascend in list order, sorted by key with equal keys in item
// order -- what std::sort of the pairs gives -- by a stable LSD radix sort of 16-bit digits over
// the keys' span (cfg 4's 262 k sub-tiles: a comparison sort cost ~7 ms of a plan-cache miss)
void sort_pairs_by_key(std::vector<std::pair<uint64_t, uint64_t>>& kv) {
    const size_t n = kv.size();
    if (n < 2) return;
    uint64_t lo = ~uint64_t(0), hi = 0;
    for (const auto& p : kv) lo = std::min(lo, p.first), hi = std::max(hi, p.first);
    std::vector<std::pair<uint64_t, uint64_t>> tmp(n);
    std::vector<uint32_t> at((size_t(1) << 16) + 1);
    const uint64_t span = hi - lo;
    for (int sh = 0; sh == 0 || (sh < 64 && (span >> sh) != 0); sh += 16) {
        std::fill(at.begin(), at.end(), 0u);
        for (const auto& p : kv) ++at[(((p.first - lo) >> sh) & 0xFFFFu) + 1];
        for (size_t d = 1; d < at.size(); ++d) at[d] += at[d - 1];
        for (const auto& p : kv) tmp[at[((p.first - lo) >> sh) & 0xFFFFu]++] = p;
        kv.swap(tmp);
    }
}

// Merges ops that continue each other: the op whose source starts where op a's source ends along
// s (a.src + a.ns * lds) and whose destination continues a's the same way (one destination
// stride further for copies, ns elements further for transposes), with the same extent along f,
// strides and flags (16-byte alignment flags aside: the merged op keeps a's, which describe its
// start and strides), joins a (then the same along f).  Same elements, same transform: only the
// op boundaries move.  Order hint: a's (the tile the merged op starts at).  `root` (optional): for every input op, the
// input op it ended up merged into (itself when it survives).
void merge_adjacent(std::vector<costa_tile_op_t>& v, int64_t E, std::vector<uint32_t>* root = nullptr) {
    std::vector<uint32_t> id(v.size());  // input index of each op of v
    for (size_t i = 0; i < v.size(); ++i) id[i] = uint32_t(i);
    if (root) {
        root->resize(v.size());
        for (size_t i = 0; i < v.size(); ++i) (*root)[i] = uint32_t(i);
    }
    if (v.size() < 2) return;
    for (int pass = 0; pass < 2; ++pass) {  // 0: along s, 1: along f
        // the ops in source order (a radix sort of (src, index)), and an open-addressing table
        // src -> the first op of that source address (std::unordered_map and std::sort cost cfg 3 /
        // cfg 4's 65 k-op lists ~5 ms of a plan-cache miss)
        std::vector<std::pair<uint64_t, uint64_t>> kv(v.size());
        for (size_t i = 0; i < v.size(); ++i) kv[i] = {v[i].src, i};
        sort_pairs_by_key(kv);
        std::vector<uint32_t> idx(v.size());
        for (size_t k = 0; k < v.size(); ++k) idx[k] = uint32_t(kv[k].second);
        int tb = 4;
        while ((size_t(1) << tb) < 2 * v.size()) ++tb;
        const size_t tmask = (size_t(1) << tb) - 1;
        std::vector<std::pair<uint64_t, uint32_t>> table(tmask + 1, {~uint64_t(0), 0u});
        auto slot_of = [&](uint64_t a) { return size_t((a * 0x9E3779B97F4A7C15ull) >> (64 - tb)); };
        for (size_t i = 0; i < v.size(); ++i) {  // ascending index: the first op of a src stays
            size_t h = slot_of(v[i].src);
            while (table[h].first != ~uint64_t(0) && table[h].first != v[i].src) h = (h + 1) & tmask;
            if (table[h].first == ~uint64_t(0)) table[h] = {v[i].src, uint32_t(i)};
        }
        auto find_src = [&](uint64_t a) -> int64_t {  // the first op at source address a, or -1
            for (size_t h = slot_of(a);; h = (h + 1) & tmask) {
                if (table[h].first == a) return int64_t(table[h].second);
                if (table[h].first == ~uint64_t(0)) return -1;
            }
        };
        std::vector<char> gone(v.size(), 0);
        for (const uint32_t i : idx) {
            if (gone[i]) continue;
            costa_tile_op_t& a = v[i];
            const bool tr = a.flags & COSTA_TILE_TRANSPOSE;
            for (;;) {
                const int64_t n = pass == 0 ? a.ns : a.nf;
                const uint64_t next_src = a.src + uint64_t(pass == 0 ? n * a.lds * E : n * E);
                const uint64_t next_dst =
                    a.dst + uint64_t(pass == 0 ? (tr ? n : n * a.ldd) * E : (tr ? n * a.ldd : n) * E);
                const int64_t nx = find_src(next_src);
                if (nx < 0 || gone[nx] || uint32_t(nx) == i) break;
                const costa_tile_op_t& b = v[size_t(nx)];
                const uint32_t vec = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
                const bool same = b.dst == next_dst && (b.flags & ~vec) == (a.flags & ~vec) && b.lds == a.lds &&
                                  b.ldd == a.ldd && (pass == 0 ? b.nf == a.nf : b.ns == a.ns);
                const int64_t total = n + (pass == 0 ? b.ns : b.nf);
                if (!same || total > (int64_t(1) << 30)) break;
                (pass == 0 ? a.ns : a.nf) = int32_t(total);
                if (!a.order) a.order = b.order;  // the merged op keeps the hint of its first tile
                gone[nx] = 1;
                if (root) (*root)[id[nx]] = id[i];
            }
        }
        size_t o = 0;
        for (size_t i = 0; i < v.size(); ++i)
            if (!gone[i]) {
                id[o] = id[i];
                v[o++] = v[i];
            }
        v.resize(o);
        id.resize(o);
    }
    if (root)  // path compression: pass 1 merged pass-0 survivors
        for (size_t i = 0; i < root->size(); ++i) {
            uint32_t r = (*root)[i];
            while ((*root)[r] != r) r = (*root)[r];
            (*root)[i] = r;
        }
}

// Ops of a list merged (merge_adjacent), keeping a merged op only when it fills the large
// shape's sub-tiles at least half along each dimension (bf x bs): a strip of one block's width
// (nf = 24 of a 64-wide sub-tile, say, a package's tiles continuing along s) would run the large
// shape a third full, slower than its tiles on the wavefront path (loopback unpack fp64 24^2
// beta != 0: 1.571 against 1.412 ms); its tiles stay apart instead.
std::vector<costa_tile_op_t> merge_filled(const std::vector<costa_tile_op_t>& cand, int64_t E, int bf, int bs) {
    std::vector<costa_tile_op_t> v = cand;
    std::vector<uint32_t> root;
    merge_adjacent(v, E, &root);
    if (v.size() == cand.size()) return v;
    std::vector<costa_tile_op_t> out;
    out.reserve(cand.size());
    std::vector<char> keep(cand.size(), 0);  // per root: the merged op is kept
    std::vector<uint32_t> count(cand.size(), 0);
    for (size_t i = 0; i < cand.size(); ++i) ++count[root[i]];
    // v holds the surviving ops in input order, i.e. in the order of their roots
    size_t k = 0;
    for (size_t i = 0; i < cand.size(); ++i) {
        if (root[i] != i) continue;
        const costa_tile_op_t& m = v[k++];
        keep[i] = count[i] == 1 || (2 * int64_t(m.nf) >= bf && 2 * int64_t(m.ns) >= bs);
        if (keep[i]) out.push_back(m);
    }
    for (size_t i = 0; i < cand.size(); ++i)
        if (!keep[root[i]]) out.push_back(cand[i]);
    return out;
}

// Only ops with equal strides can continue each other: block-cyclic layouts have one stride per
// local matrix, while a custom layout whose blocks are separate buffers has one per block (cfg 5:
// hundreds), whose tiles practically never continue across blocks.  Lists with more than 16
// distinct source strides skip the merge (cfg 5's 245 k ops: the merge pass cost 2x build_work).
bool few_strides(const std::vector<costa_tile_op_t>& ops) {
    int32_t seen[16];
    int k = 0;
    for (const auto& o : ops) {
        bool found = false;
        for (int i = 0; i < k && !found; ++i) found = seen[i] == o.lds;
        if (found) continue;
        if (k == 16) return false;
        seen[k++] = o.lds;
    }
    return true;
}

// runs fn(begin, end) over [0, n) on up to 8 host threads (one when n < min_items)
template <typename F>
void host_parallel(size_t n, F fn, size_t min_items = 32768) {
    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t T = n < min_items ? 1 : std::min<size_t>(8, hw);
    if (T == 1) return fn(size_t(0), n);
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> err(T);
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            try {
                fn(n * t / T, n * (t + 1) / T);
            } catch (...) {
                err[t] = std::current_exception();
            }
        });
    for (auto& x : th) x.join();
    for (auto& e : err)
        if (e) std::rethrow_exception(e);
}
}  // namespace

namespace {
// Destination-block groups (r5, tile_kernels.hip cblock_kernel).  Among the ops bound for the
// wavefront path, those whose destination footprints (same leading dimension R) overlap or touch
// form components; a component whose ops tile R x K elements exactly -- whole columns of a
// buffer whose leading dimension is R: a custom layout's own block buffer (cfg 5), or several of
// them back to back -- is one contiguous destination range, written by one workgroup in 16-byte
// vectors instead of one element a lane per wavefront piece.  Components above the workgroup's
// budget (cblock_max_elems) are cut into column bands, their ops cut at the band edges (a
// sub-rectangle of a tile op is a tile op).  Ops of a component must share one transform (flags
// apart from the vector bits).  Emitted into `ordered` as [header, ops...] per group (header: src
// = number of ops, dst = the range, nf = R, ns = K, flags = the transform); `work` gets the
// header indices in destination order; the grouped ops leave `wave_ops`.  COSTA_CBLOCK=0
// (tuning): off.
// the destination-block groups apply to this list (cblock_groups' own conditions, apart from the
// list's length)
bool cblock_enabled(costa_dtype_t dtype, list_kind kind) {
    static const int on = [] {
        const char* s = tuning_env("COSTA_CBLOCK");
        return s ? std::atoi(s) : 1;
    }();
    const bool real = dtype == COSTA_FLOAT || dtype == COSTA_DOUBLE || dtype == COSTA_INT32;
    return on && real && kind != list_pack;
}

int64_t cblock_groups(costa_dtype_t dtype, std::vector<const costa_tile_op_t*>& wave_ops, list_kind kind,
                      std::vector<costa_tile_op_t>& ordered, std::vector<uint64_t>& work, int64_t& lds,
                      int& map, const std::vector<costa_tile_op_t>& ops, device_section* dev) {
    static const int on = [] {
        const char* s = tuning_env("COSTA_CBLOCK");
        return s ? std::atoi(s) : 1;
    }();
    // COSTA_CB_BANDS (tuning): 1 XCD column bands for every list, 0 never, -1 (default) as below
    static const int bands_env = [] {
        const char* s = tuning_env("COSTA_CB_BANDS");
        return s ? std::atoi(s) : -1;
    }();
    lds = 0;
    map = cb_round_robin;
    // COSTA_PLAN_TRACE=1: the phases of the group builder (stderr)
    static const bool trace = std::getenv("COSTA_PLAN_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    double lap_ms[7] = {0, 0, 0, 0, 0, 0, 0};  // candidates, sort, components, check, groups, order, emit
    auto lap = [&](int k) {
        if (trace) lap_ms[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    // real types (complex elements are on the large shapes wherever it matters: cfg 4)
    const bool real = dtype == COSTA_FLOAT || dtype == COSTA_DOUBLE || dtype == COSTA_INT32;
    if (!on || !real || kind == list_pack || wave_ops.size() < 2) return 0;
    const int64_t E = int64_t(dtype_size(dtype));
    const uint32_t vec_bits = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    // a range of n elements starting off the 16-byte grid spans up to n + V - 1 elements of
    // whole vectors: the workgroup's kCblockChunks vectors a thread must cover that
    const int64_t budget = cblock_max_elems(E) - (16 / E - 1);
    // on the GPU (device_lists.hip) for long lists: the same groups, order and bytes
    const int lb_mode = list_builder_mode();
    if (dev && dev->device >= 0 && (dev->force || lb_mode == 2 || (lb_mode == 1 && wave_ops.size() >= kDeviceGroupsMin))) {
        std::vector<uint32_t> wave(wave_ops.size());
        for (size_t i = 0; i < wave_ops.size(); ++i) wave[i] = uint32_t(wave_ops[i] - ops.data());
        std::vector<char> taken;
        const int64_t ng = cblock_groups_device(E, budget, vec_bits, bands_env, ops, wave, ordered.size(), *dev,
                                                taken, lds, map);
        if (ng >= 0) {
            if (ng > 0) {
                dev->at_work = work.size();
                size_t o = 0;
                for (size_t i = 0; i < wave_ops.size(); ++i)
                    if (!taken[i]) wave_ops[o++] = wave_ops[i];
                wave_ops.resize(o);
                g_stats.device_lists++;
            }
            if (trace)
                std::fprintf(stderr, "[costa groups] %lld groups built on the GPU in %.2f ms\n", (long long)ng,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            return ng;
        }
    }
    struct cand {
        uint64_t lo, hi;
        int32_t ldd;
        uint32_t i;
    };
    std::vector<cand> cs;
    cs.reserve(wave_ops.size());
    for (uint32_t i = 0; i < wave_ops.size(); ++i) {
        const costa_tile_op_t& op = *wave_ops[i];
        if (op.nf <= 0 || op.ns <= 0 || op.ldd <= 0 || op.dst % uint64_t(E) != 0) continue;
        const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
        const int64_t run = tr ? op.ns : op.nf, runs = tr ? op.nf : op.ns;
        if (run > op.ldd || op.ldd > budget) continue;
        cs.push_back({op.dst, op.dst + uint64_t(((runs - 1) * int64_t(op.ldd) + run) * E), op.ldd, i});
    }
    if (cs.size() < 2) return 0;
    lap(0);
    // order by (ldd, lo): stable LSD radix sorts, lo (element offsets from the lowest) first, then
    // ldd (<= budget); a comparison sort of cfg 5's 245 k candidates cost ~10 ms of a plan miss
    {
        uint64_t lo_min = ~uint64_t(0), lo_max = 0;
        for (const auto& c : cs) lo_min = std::min(lo_min, c.lo), lo_max = std::max(lo_max, c.lo);
        std::vector<cand> tmp(cs.size());
        constexpr int B = 16;  // 2 passes for cfg 5's 1 GiB arena, 1 for the leading dimensions
        std::vector<uint32_t> at((size_t(1) << B) + 1);
        auto pass = [&](auto digit) {
            std::fill(at.begin(), at.end(), 0u);
            for (const auto& c : cs) ++at[digit(c) + 1];
            for (size_t d = 1; d < at.size(); ++d) at[d] += at[d - 1];
            for (const auto& c : cs) tmp[at[digit(c)]++] = c;
            cs.swap(tmp);
        };
        const uint64_t span = (lo_max - lo_min) / uint64_t(E);
        for (int sh = 0; sh == 0 || (sh < 64 && (span >> sh) != 0); sh += B)
            pass([&](const cand& c) { return size_t(((c.lo - lo_min) / uint64_t(E) >> sh) & ((1u << B) - 1)); });
        for (int sh = 0; sh == 0 || (sh < 31 && (uint64_t(budget) >> sh) != 0); sh += B)
            pass([&](const cand& c) { return size_t((uint32_t(c.ldd) >> sh) & ((1u << B) - 1)); });
    }
    lap(1);
    // components: runs of candidates (one leading dimension) whose footprints overlap or touch
    struct comp {
        size_t a, b;
    };
    std::vector<comp> comps;
    for (size_t a = 0; a < cs.size();) {
        size_t b = a + 1;
        uint64_t hi = cs[a].hi;
        while (b < cs.size() && cs[b].ldd == cs[a].ldd && cs[b].lo <= hi) hi = std::max(hi, cs[b].hi), ++b;
        if (b - a >= 2) comps.push_back({a, b});
        a = b;
    }
    lap(2);
    // per component (host threads): does it tile its R x K range exactly, and how many groups
    // (column bands of at most `budget` elements) it makes
    struct cinfo {
        int64_t K = 0, KB = 0;
        uint64_t n_groups = 0;
        uint32_t fl = 0;
    };
    std::vector<cinfo> ci(comps.size());
    // (gathering the candidates' ops into sorted order first made the passes below no faster on
    // the box: tiling check + group table + emission 16.5 against 12.4 ms, profiles/r6g/)
    auto op_of = [&](size_t k) -> const costa_tile_op_t& { return *wave_ops[cs[k].i]; };
    host_parallel(comps.size(), [&](size_t x0, size_t x1) {
        std::vector<uint64_t> corner;
        for (size_t x = x0; x < x1; ++x) {
            const size_t a0 = comps[x].a, b = comps[x].b;
            const int64_t R = cs[a0].ldd;
            const uint64_t base = cs[a0].lo;
            const uint32_t fl = op_of(a0).flags & ~vec_bits;
            int64_t area = 0, K = 0;
            bool ok = true;
            for (size_t k = a0; k < b && ok; ++k) {
                const costa_tile_op_t& op = op_of(k);
                const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
                const int64_t run = tr ? op.ns : op.nf, runs = tr ? op.nf : op.ns;
                const int64_t e = int64_t(op.dst - base) / E;
                ok = (op.flags & ~vec_bits) == fl && e % R + run <= R;
                area += run * runs;
                K = std::max(K, e / R + runs);
            }
            if (!ok || area != R * K || K > INT32_MAX) continue;
            // ... and tile it exactly: with the areas adding up to R x K, the ops tile the range
            // iff every corner point occurs an even number of times, the range's own four corners
            // apart, which occur once ("perfect rectangle").  Overlapping ops whose areas happen to
            // add up would leave elements no op writes, and the group kernel would store its
            // uninitialised LDS there (costa_hip_execute_tiles takes caller ops).
            corner.clear();
            const uint64_t W = uint64_t(K) + 1;
            for (size_t k = a0; k < b; ++k) {
                const costa_tile_op_t& op = op_of(k);
                const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
                const uint64_t run = uint64_t(tr ? op.ns : op.nf), runs = uint64_t(tr ? op.nf : op.ns);
                const uint64_t e = (op.dst - base) / uint64_t(E), r0 = e % uint64_t(R), c0 = e / uint64_t(R);
                for (const uint64_t r : {r0, r0 + run})
                    for (const uint64_t c : {c0, c0 + runs}) corner.push_back(r * W + c);
            }
            std::sort(corner.begin(), corner.end());
            const uint64_t ur = uint64_t(R), uk = uint64_t(K), want[4] = {0, uk, ur * W, ur * W + uk};
            int n_odd = 0;
            for (size_t k = 0; k < corner.size() && ok;) {
                size_t m = k;
                while (m < corner.size() && corner[m] == corner[k]) ++m;
                if ((m - k) & 1) ok = n_odd < 4 && corner[k] == want[n_odd++];
                k = m;
            }
            if (!ok || n_odd != 4) continue;
            const int64_t KB = std::max<int64_t>(1, budget / R);
            ci[x] = {K, KB, uint64_t((K + KB - 1) / KB), fl};
        }
    }, 4096);
    lap(3);
    std::vector<uint64_t> g_at(comps.size() + 1, 0);
    for (size_t x = 0; x < comps.size(); ++x) g_at[x + 1] = g_at[x] + ci[x].n_groups;
    const size_t ng = size_t(g_at.back());
    if (ng == 0) return 0;
    // per group (host threads): its range, its op count (an op cut at the band edges counts once
    // per band), the smallest locality hint of its ops (0: one lacks a hint)
    struct group {
        uint64_t dst;
        uint32_t comp, band, n_ops, hint;
    };
    std::vector<group> gs(ng);
    std::vector<char> taken(wave_ops.size(), 0);
    auto band_cols = [&](size_t x, uint32_t band, int64_t& cb0, int64_t& cb1) {
        cb0 = int64_t(band) * ci[x].KB;
        cb1 = std::min(ci[x].K, cb0 + ci[x].KB);
    };
    host_parallel(comps.size(), [&](size_t x0, size_t x1) {
        for (size_t x = x0; x < x1; ++x) {
            if (ci[x].n_groups == 0) continue;
            const size_t a0 = comps[x].a, b = comps[x].b;
            const int64_t R = cs[a0].ldd;
            const uint64_t base = cs[a0].lo;
            for (uint32_t band = 0; band < ci[x].n_groups; ++band) {
                int64_t cb0, cb1;
                band_cols(x, band, cb0, cb1);
                group& g = gs[size_t(g_at[x]) + band];
                g = {base + uint64_t(cb0 * R * E), uint32_t(x), band, 0, UINT32_MAX};
                for (size_t k = a0; k < b; ++k) {
                    const costa_tile_op_t& op = op_of(k);
                    const int64_t c0 = int64_t(op.dst - base) / E / R;
                    const int64_t runs = (op.flags & COSTA_TILE_TRANSPOSE) ? op.nf : op.ns;
                    if (std::max(cb0, c0) >= std::min(cb1, c0 + runs)) continue;
                    ++g.n_ops;
                    g.hint = op.order ? std::min(g.hint, op.order) : 0;
                }
            }
        }
    }, 4096);
    // (one thread: the grouped ops are scattered over the list, and threads marking them shared
    // cache lines)
    for (size_t x = 0; x < comps.size(); ++x)
        if (ci[x].n_groups)
            for (size_t k = comps[x].a; k < comps[x].b; ++k) taken[cs[k].i] = 1;
    lap(4);
    // destination order: a stable radix sort of the groups by range offset
    std::vector<uint32_t> order(ng);
    {
        uint64_t lo = ~uint64_t(0), hi = 0;
        for (const auto& g : gs) lo = std::min(lo, g.dst), hi = std::max(hi, g.dst);
        std::vector<uint32_t> tmp(ng);
        for (size_t g = 0; g < ng; ++g) order[g] = uint32_t(g);
        constexpr int B = 16;
        std::vector<uint32_t> at((size_t(1) << B) + 1);
        const uint64_t span = (hi - lo) / uint64_t(E);
        for (int sh = 0; sh == 0 || (sh < 64 && (span >> sh) != 0); sh += B) {
            auto digit = [&](uint32_t g) { return size_t(((gs[g].dst - lo) / uint64_t(E) >> sh) & ((1u << B) - 1)); };
            std::fill(at.begin(), at.end(), 0u);
            for (const uint32_t g : order) ++at[digit(g) + 1];
            for (size_t d = 1; d < at.size(); ++d) at[d] += at[d - 1];
            for (const uint32_t g : order) tmp[at[digit(g)]++] = g;
            order.swap(tmp);
        }
    }
    bool any_tr = false;
    for (const auto& g : gs) any_tr = any_tr || (ci[g.comp].fl & COSTA_TILE_TRANSPOSE);
    map = any_tr ? cb_xcd_chunks : cb_round_robin;
    bool hints = true;
    for (const auto& g : gs) hints = hints && g.hint != 0 && g.hint != UINT32_MAX;
    // XCD column bands for copy-only lists (r6, COSTA_CB_BANDS=0 / 1 (tuning): never / always):
    // the groups in the planner's column-major order of their first target tile are cut into 8
    // slices of the kernel's sizes (xcd_slice_order), slice x -- one band of target columns --
    // walked by XCD x in destination order.  A source block split by a target block-row boundary
    // is then read by two groups of one XCD about 1/8 of a block-row of its traffic apart, while
    // the line they share is still in its L2: cfg 5 'N' reads 1.46x -> 1.03x their bytes, and
    // with the 16-byte chunk loads of copy groups 0.436 -> 0.427 ms (each alone: +1 %, +1 %;
    // profiles/r6c/, r6d/).  Transposing lists keep the 4-group XCD chunks ('T' 0.600 against
    // 0.619 ms with bands).
    const bool bands = bands_env == 1 || (bands_env == -1 && !any_tr);
    if (bands && ng >= 16 && hints) {
        // (stable counting sorts: by hint, 2 x 16-bit digits; then the slices, 8 buckets)
        const size_t per = ng / 8, rem = ng % 8;
        std::vector<uint32_t> by(ng), tmp(ng), at16((size_t(1) << 16) + 1);
        for (size_t i = 0; i < ng; ++i) by[i] = uint32_t(i);
        for (int sh = 0; sh < 32; sh += 16) {
            std::fill(at16.begin(), at16.end(), 0u);
            for (const uint32_t g : by) ++at16[((gs[g].hint >> sh) & 0xFFFFu) + 1];
            for (size_t d = 1; d < at16.size(); ++d) at16[d] += at16[d - 1];
            for (const uint32_t g : by) tmp[at16[(gs[g].hint >> sh) & 0xFFFFu]++] = g;
            by.swap(tmp);
        }
        std::vector<uint8_t> band(ng);
        for (size_t k = 0; k < ng; ++k)
            band[by[k]] = uint8_t(k < rem * (per + 1) ? k / (per + 1) : rem + (k - rem * (per + 1)) / per);
        uint32_t at8[9] = {0};
        for (const uint32_t g : order) ++at8[band[g] + 1];
        for (int d = 1; d < 9; ++d) at8[d] += at8[d - 1];
        for (const uint32_t g : order) tmp[at8[band[g]]++] = g;
        order.swap(tmp);
        map = cb_xcd_bands;
    }
    lap(5);
    // [header, ops...] per group in that order, each op cut at its band's edges (a sub-rectangle
    // of a tile op is a tile op), written straight into their places (host threads)
    const size_t base_at = ordered.size();
    std::vector<uint64_t> at(ng + 1, 0);
    for (size_t q = 0; q < ng; ++q) at[q + 1] = at[q] + 1 + gs[order[q]].n_ops;
    size_t rest = 0;  // the remaining wavefront ops' pieces follow: room for most of them
    for (size_t i = 0; i < wave_ops.size(); ++i) rest += !taken[i];
    ordered.reserve(base_at + size_t(at[ng]) + 4 * rest + 1024);
    ordered.resize(base_at + size_t(at[ng]));
    work.reserve(work.size() + ng);
    for (size_t q = 0; q < ng; ++q) {
        work.push_back(uint64_t(base_at + at[q]));
        const group& g = gs[order[q]];
        int64_t cb0, cb1;
        band_cols(g.comp, g.band, cb0, cb1);
        lds = std::max(lds, int64_t(cs[comps[g.comp].a].ldd | 1) * (cb1 - cb0));
    }
    host_parallel(ng, [&](size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; ++q) {
            const group& g = gs[order[q]];
            const size_t x = g.comp, a0 = comps[x].a, b = comps[x].b;
            const int64_t R = cs[a0].ldd;
            const uint64_t base = cs[a0].lo;
            int64_t cb0, cb1;
            band_cols(x, g.band, cb0, cb1);
            costa_tile_op_t* out = &ordered[base_at + size_t(at[q])];
            costa_tile_op_t h{};
            h.src = g.n_ops;
            h.dst = g.dst;
            h.nf = int32_t(R);
            h.ns = int32_t(cb1 - cb0);
            h.ldd = int32_t(R);
            h.flags = ci[x].fl;
            *out++ = h;
            for (size_t k = a0; k < b; ++k) {
                costa_tile_op_t op = op_of(k);
                const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
                const int64_t c0 = int64_t(op.dst - base) / E / R;
                const int64_t runs = tr ? op.nf : op.ns;
                const int64_t lo = std::max(cb0, c0), up = std::min(cb1, c0 + runs);
                if (lo >= up) continue;
                const int64_t d0 = lo - c0, dn = up - lo;  // destination columns of the op kept
                op.dst += uint64_t(d0 * R * E);
                if (tr) {  // destination columns = source f
                    op.src += uint64_t(d0 * E);
                    op.nf = int32_t(dn);
                } else {  // destination columns = source s
                    op.src += uint64_t(d0 * int64_t(op.lds) * E);
                    op.ns = int32_t(dn);
                }
                *out++ = op;
            }
        }
    }, 4096);
    size_t o = 0;
    for (size_t i = 0; i < wave_ops.size(); ++i)
        if (!taken[i]) wave_ops[o++] = wave_ops[i];
    wave_ops.resize(o);
    if (trace) {
        lap(6);
        std::fprintf(stderr,
                     "[costa groups] %zu candidates, %zu components, %zu groups: candidates %.2f ms, sort %.2f, "
                     "components %.2f, tiling check %.2f, group table %.2f, order %.2f, emit %.2f\n",
                     cs.size(), comps.size(), ng, lap_ms[0], lap_ms[1] - lap_ms[0], lap_ms[2] - lap_ms[1],
                     lap_ms[3] - lap_ms[2], lap_ms[4] - lap_ms[3], lap_ms[5] - lap_ms[4], lap_ms[6] - lap_ms[5]);
    }
    return int64_t(ng);
}

struct wave_knobs {  // defaults, overridable for tuning runs
    int policy = 2;  // COSTA_WAVE_POLICY 1: every op below the large threshold takes the wave
                     // path; 2: also large ops that are not 16-byte aligned on both sides, up to
                     // kUnalignedWaveCap large sub-tiles of data (r11: cfg 5 geometry with
                     // doubled edges 3.41 -> 4.14 TB/s 'N', 3.47 -> 3.88 'T', the rest
                     // unchanged; profiles/r11/c5_align_policy*.log).  Bigger unaligned ops stay
                     // on the large shape (its guarded path): cut into wavefront pieces, a
                     // 16384^2 fp32 op would become ~350 k pieces of host and device list.
    int skew_xcd = -1;   // COSTA_SKEW_XCD=F (tuning): F skew sub-tiles continuing each other's
                         // source rows on one XCD (one L2) at the same time; -1 (default):
                         // kSkewWideGroup for lists on the wide skew variant, else none
    int panel_rows = 0;  // COSTA_PANEL_ROWS (tuning): rows per destination panel of the
                         // destination-ordered sub-tiles; 0: 128 KiB of rows (default), -1: none
    int large_sort = 3;  // COSTA_LARGE_SORT 1: large ops in the order of the planner's locality
                         // hint (column-major target order: consecutive ops continue down the
                         // same target columns, so the write stream is sequential in aggregate);
                         // 0: list order (the reference's message order: target row-major, every
                         // op a new target column at the same in-column offset, which camps on
                         // HBM channels; tools/copy_ceiling.hip "pat ... ord-1" 6.27 against 5.64
                         // TB/s, "segcamp" 4.4-4.9 against 6.4); 2: 1, then the sub-tiles by
                         // the address of their first destination element (one sub-tile-wide
                         // band of target columns at a time, instead of an op's 2-4 sub-tiles
                         // side by side); 3 (default): 2 for lists whose shaped ops all transpose
                         // 4- or 8-byte elements (fp64 / c64 'T' 16384^2: 0.710 against 0.747 ms
                         // with 256^2 blocks, 0.709 against 0.797 with 512^2; fp32 with its
                         // 128 x 128 sub-tiles 0.366 against 0.396 with 256^2, 0.366 against
                         // 0.454 with 512^2), else 1 (c128 with 128^2 blocks: 2.87 against 2.27
                         // ms; copy lists untested under 2; profiles/r2/order/)
    int copy_granule = 1;  // copy ops into destinations off the 64-byte grid cut at each column's
                           // granules (granule_split; r6: fp64 16384^2 'N' ldc + 1 / + 2 / + 3
                           // 0.89 / 0.79 / 0.93 -> 0.76 / 0.76 / 0.74 ms, fp32 + 1 0.51 -> 0.41,
                           // int32 + 3 0.51 -> 0.41, 16-byte aligned fp32 + 4 level; profiles/r6b/);
                           // COSTA_COPY_GRANULE=0 (tuning): off
    int force_sq = 0;   // COSTA_FORCE_SQ=1 (tuning): transposing lists of fp64 / c64 / c128 take the
                        // square sub-tile whatever their ops' size
    int merge = 2;      // COSTA_MERGE=0: ops that continue each other are not merged, 1: only
                        // ops below half a large sub-tile (r3); 2 (default): every op (tuning; the
                        // skew list always merges)
    int xcd_bands = 1;  // COSTA_XCD_BANDS=k: destination-ordered wavefront lists in 8 k column
                        // bands, k per XCD (xcd_bands); 0: off.  cfg 5 'N' 0.476 -> 0.446 ms with
                        // k = 1 (2 / 4 / 16: 0.464 / 0.475 / 0.490), 'T' equal; through the
                        // loopback exchange unpack 'N' 0.609 -> 0.592, 'T' 1.016 -> 0.960
                        // (profiles/r3b/README.md §bands)
    int sort = 5;    // COSTA_TINY_SORT 0: list order, 1: by source, 2: by destination address,
                     // 3: by the planner's locality hint (costa_tile_op_t::order), 4: 3 for
                     // copy-only lists, 2 for lists that transpose (cfg 5 'T' 3.88 against
                     // 3.79 TB/s, 'N' equal; profiles/r11/c5_env.log), else as 2; 5 (default):
                     // pack lists by source address (their destinations, the dense package,
                     // are contiguous per op in any order), every other list by destination
                     // address.  cfg 5 under 5 against 4 on one lease (tools/c5_sort_probe.py,
                     // profiles/r2c/c5_sort.log): local 'N' 0.497 / 0.499-0.502 ms, 'T' equal;
                     // with every tile through the exchange (COSTA_LOOPBACK=1) 'N' pack 0.557-0.561
                     // / 0.596-0.600, unpack 0.556-0.558 / 0.606-0.610, 'T' pack 0.725-0.729 /
                     // 0.751-0.761, unpack equal
};
// f-neighbour skew sub-tiles grouped per XCD on the wide variant (fp32 16384^2 'T', both sides
// lld 16385: 0.453 / 0.440 / 0.428 / 0.419-0.424 ms with groups of 1 / 2 / 4 / 8; profiles/r3b/README.md §skew)
constexpr int64_t kSkewWideGroup = 8;
const wave_knobs& knobs() {
    static wave_knobs k = [] {
        wave_knobs x;
        if (const char* s = tuning_env("COSTA_WAVE_POLICY")) x.policy = std::atoi(s) == 1 ? 1 : 2;
        if (const char* s = tuning_env("COSTA_TINY_SORT")) x.sort = std::max(0, std::min(5, std::atoi(s)));
        if (const char* s = tuning_env("COSTA_LARGE_SORT")) x.large_sort = std::max(0, std::min(3, std::atoi(s)));
        if (const char* s = tuning_env("COSTA_PANEL_ROWS")) x.panel_rows = std::max(-1, std::atoi(s));
        if (const char* s = tuning_env("COSTA_SKEW_XCD")) x.skew_xcd = std::max(-1, std::atoi(s));
        if (const char* s = tuning_env("COSTA_XCD_BANDS")) x.xcd_bands = std::atoi(s);
        if (const char* s = tuning_env("COSTA_MERGE")) x.merge = std::atoi(s);
        if (const char* s = tuning_env("COSTA_FORCE_SQ")) x.force_sq = std::atoi(s);
        if (const char* s = tuning_env("COSTA_COPY_GRANULE")) x.copy_granule = std::atoi(s);
        return x;
    }();
    return k;
}
}  // namespace

// Copies into destinations off the 64-byte grid (a ScaLAPACK lld that is not a multiple of 64
// bytes, or a sub-matrix offset): the large copy shape writes each destination column in 1 KiB
// segments from the op's first row, so every segment boundary inside a column is a 64-byte
// granule shared by two workgroups, which HBM services as a read-modify-write.  Cut
// instead at each column's own granules: the op's columns are split by their residue modulo the
// period p after which a column starts at the same granule offset again (p * ldd * E = 0 mod 64),
// so each part has one offset eps for every column; its first G - eps rows (G = 64 / E elements:
// the head of each column's first granule) become an op of their own (the wavefront path), and
// the rest starts every column on a granule boundary, its segments whole granules.  Sub-rectangles
// of a copy op are copy ops: the same elements, the same transform; only the op boundaries move.
// Ops below `min_elems` (the wavefront path anyway) and transposing ops (the skew shape, §3b) stay
// as they are.  -> true when `out` holds a split list
bool granule_split(const std::vector<costa_tile_op_t>& ops, int64_t E, int64_t min_elems,
                   std::vector<costa_tile_op_t>& out) {
    const int64_t G = 64 / E;
    auto split_it = [&](const costa_tile_op_t& op) {
        if (G <= 1 || (op.flags & COSTA_TILE_TRANSPOSE) || op.dst % uint64_t(E) != 0) return false;
        if (int64_t(op.nf) * op.ns < min_elems || op.nf < 2 * G) return false;
        if (int64_t(std::max(op.lds, op.ldd)) * 64 > INT32_MAX) return false;  // p * ld must fit
        return op.dst % 64 != 0 || (uint64_t(op.ldd) * uint64_t(E)) % 64 != 0;
    };
    bool any = false;
    for (const auto& op : ops) any = any || split_it(op);
    if (!any) return false;
    out.clear();
    out.reserve(ops.size() + 64);
    const uint32_t vec_bits = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    for (const auto& op : ops) {
        if (!split_it(op)) {
            out.push_back(op);
            continue;
        }
        const uint64_t row_bytes = uint64_t(op.ldd) * uint64_t(E);
        const int64_t p = 64 / int64_t(std::gcd(row_bytes % 64 == 0 ? uint64_t(64) : row_bytes % 64, uint64_t(64)));
        // 4-byte sources are read as 16-byte vectors at dword alignment (build_work: mis)
        const uint32_t keep_vs = E == 4 ? (op.flags & COSTA_TILE_VEC_SRC) : 0u;
        for (int64_t r = 0; r < std::min<int64_t>(p, op.ns); ++r) {
            costa_tile_op_t part = op;
            part.src = op.src + uint64_t(r * int64_t(op.lds) * E);
            part.dst = op.dst + uint64_t(r * int64_t(op.ldd) * E);
            part.ns = int32_t((op.ns - r + p - 1) / p);
            part.lds = int32_t(int64_t(op.lds) * p);
            part.ldd = int32_t(int64_t(op.ldd) * p);
            const int64_t eps = int64_t(part.dst % 64) / E;
            const int64_t h = eps > 0 ? std::min<int64_t>(op.nf, G - eps) : 0;
            if (h > 0) {  // the head of each column's first granule
                costa_tile_op_t head = part;
                head.nf = int32_t(h);
                head.flags = (op.flags & ~vec_bits) | vec_flags(head.src, head.lds, head.dst, head.ldd, E) | keep_vs;
                out.push_back(head);
            }
            if (h < op.nf) {
                costa_tile_op_t body = part;
                body.src += uint64_t(h * E);
                body.dst += uint64_t(h * E);
                body.nf = int32_t(op.nf - h);
                body.flags = (op.flags & ~vec_bits) | vec_flags(body.src, body.lds, body.dst, body.ldd, E) | keep_vs;
                out.push_back(body);
            }
        }
    }
    return true;
}

work_split build_work(costa_dtype_t dtype, const std::vector<costa_tile_op_t>& ops_in,
                      std::vector<costa_tile_op_t>& ordered, std::vector<uint64_t>& work,
                      list_kind kind, device_section* dev, bool dst_order) {
    const bool pack_list = kind == list_pack, local = kind == list_local;
    // Sources off the 16-byte grid: 4-byte elements are read as 16-byte vectors anyway (dword
    // alignment suffices for global_load_dwordx4): fp32 16384^2 'T' with lld 16386 0.405 against
    // 0.499 ms element by element; 8-byte elements stay element-wise (0.794 against 0.755 ms);
    // misaligned 16-byte stores lost for both (tools/unaligned_mis.sh, profiles/r3/).
    // COSTA_MISALIGNED_VEC (tuning): bit 0 destinations, bit 1 sources, for every element size.
    static const int mis_env = [] {
        const char* s = tuning_env("COSTA_MISALIGNED_VEC");
        return s ? std::atoi(s) : -1;
    }();
    // (by default only for ops of at least one large sub-tile: smaller ones keep their class)
    const int mis = mis_env >= 0 ? mis_env : dtype_size(dtype) == 4 ? 2 : 0;
    // tiles of one local matrix that continue each other in source and destination become one op
    // (a 16384^2 'T' with 24^2 blocks on one rank: one op on the large shape instead of 466 k
    // wavefront tiles)
    const wave_knobs& kn0 = knobs();
    // COSTA_PLAN_TRACE=1: where build_work spends its time (stderr; get_plan traces the whole miss)
    static const bool trace = std::getenv("COSTA_PLAN_TRACE") != nullptr;
    const auto bw0 = std::chrono::steady_clock::now();
    double bw_t[4] = {0, 0, 0, 0};  // classify + shaped lists, groups, wavefront order, pieces
    double sub_t[3] = {0, 0, 0};    // ... of the first: merge, vector flags + granule cut, classify
    auto lap = [&](int k) {
        if (!trace) return;
        const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - bw0).count();
        bw_t[k] = t;
    };
    auto mark = [&](int k) {
        if (trace) sub_t[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - bw0).count();
    };
    std::vector<costa_tile_op_t> ops_merged;
    const std::vector<costa_tile_op_t>* ops_src = &ops_in;
    if (kn0.merge && ops_in.size() > 1 && few_strides(ops_in)) {
        shape_dims sh0;
        tile_shapes(dtype, any_transpose(ops_in), &sh0);
        // every op is a candidate, large ones included (r4): blocks that do not fill the
        // sub-tiles then run as whole merged ops (16384^2 'T' on one rank: c128 80^2 / 96^2
        // 2.919 / 2.554 -> 2.101 / 2.103 ms, fp64 96^2 0.800 -> 0.699, 100^2 0.947 -> 0.700, 80^2
        // beta != 0 1.212 -> 1.030; filled sizes unchanged; profiles/r4s/).  COSTA_MERGE=1
        // (tuning): small ops only, as in r3
        const int64_t half_large = kn0.merge == 1 ? int64_t(sh0.cf) * sh0.cs / 2 : INT64_MAX;
        std::vector<costa_tile_op_t> cand;  // the ops that may merge (the rest: ops_merged as they are)
        for (const auto& op : ops_in)
            (int64_t(op.nf) * op.ns < half_large ? cand : ops_merged).push_back(op);
        const size_t n_cand0 = cand.size();
        cand = merge_filled(cand, int64_t(dtype_size(dtype)), sh0.cf, sh0.cs);
        if (cand.size() < n_cand0) {
            ops_merged.insert(ops_merged.end(), cand.begin(), cand.end());
            ops_src = &ops_merged;
        }
    }
    mark(0);
    std::vector<costa_tile_op_t> ops_mis;
    bool mis_any = false;  // (the list is copied only when some op gains a flag: cfg 5's 245 k
                           // small ops gain none, and the copy cost a plan-cache miss ~2 ms)
    if (mis) {
        const uint64_t E = dtype_size(dtype);
        shape_dims shm;
        tile_shapes(dtype, any_transpose(ops_in), &shm);
        const int64_t min_elems = mis_env >= 0 ? 0 : int64_t(shm.cf) * shm.cs;
        auto gain = [&](const costa_tile_op_t& op) {
            uint32_t f = 0;
            if (int64_t(op.nf) * op.ns < min_elems) return f;
            if ((mis & 1) && op.dst % 4 == 0 && (uint64_t(op.ldd) * E) % 4 == 0) f |= COSTA_TILE_VEC_DST;
            if ((mis & 2) && op.src % 4 == 0 && (uint64_t(op.lds) * E) % 4 == 0) f |= COSTA_TILE_VEC_SRC;
            return f & ~op.flags;
        };
        for (const auto& op : *ops_src) mis_any = mis_any || gain(op) != 0;
        if (mis_any) {
            ops_mis = *ops_src;
            for (auto& op : ops_mis) op.flags |= gain(op);
        }
    }
    const std::vector<costa_tile_op_t>* ops_pre = mis_any ? &ops_mis : ops_src;
    std::vector<costa_tile_op_t> ops_gran;
    if (kn0.copy_granule) {
        shape_dims shg;
        tile_shapes(dtype, any_transpose(ops_in), &shg);
        if (granule_split(*ops_pre, int64_t(dtype_size(dtype)), int64_t(shg.cf) * shg.cs / 2, ops_gran))
            ops_pre = &ops_gran;
    }
    const std::vector<costa_tile_op_t>& ops = *ops_pre;
    mark(1);
    const bool tr_shape = any_transpose(ops);
    shape_dims sh;
    tile_shapes(dtype, tr_shape, &sh);
    const int64_t E = int64_t(dtype_size(dtype));
    const wave_knobs& kn = knobs();
    ordered.clear();
    work.clear();
    std::vector<const costa_tile_op_t*> wave_ops;  // ops for the wavefront path, in list order
    wave_ops.reserve(ops.size());
    const uint32_t vec_both = COSTA_TILE_VEC_SRC | COSTA_TILE_VEC_DST;
    const int64_t sub_elems = int64_t(sh.cf) * sh.cs;                // one large class unit
    const int64_t med_elems = int64_t(sh.bf_m) * sh.bs_m;            // one medium sub-tile (0: none)
    // classify: wavefront path, the medium shape (aligned ops of at least half its sub-tile, in
    // lists that transpose) or the large shape
    // (a medium launch of fewer than kMinMediumOps ops costs more than it saves: it runs ahead of
    // the wavefront kernel, not beside it; cfg 5 'T' with its 969 medium ops 0.802 against 0.791
    // ms without, profiles/r2/shapes/ab_medium_cfg5T.log)
    constexpr size_t kMinMediumOps = 4096;
    std::vector<uint8_t> cls(ops.size(), 3);  // 0 large, 1 medium, 2 wavefront, 3 empty
    auto is_large = [&](const costa_tile_op_t& op, int64_t lo) {
        const int64_t elems = int64_t(op.nf) * op.ns;
        const bool aligned = (op.flags & vec_both) == vec_both;
        bool large = 2 * elems >= lo;
        if (kn.policy == 2 && !aligned && elems <= kUnalignedWaveCap * sub_elems) large = false;
        return large && !is_tiny(op, E, local);
    };
    // A transposing list whose large ops all fit the square variant of the large shape (bf_q x
    // bs_q) runs them on it: one sub-tile per op instead of a half-filled large one (fp64 / c64 /
    // c128 64^2 blocks).  Without a medium tier (complex types) the large class then starts at
    // half a square sub-tile.
    const int64_t q_elems = int64_t(sh.bf_q) * sh.bs_q;
    const int64_t q_lo = med_elems > 0 ? sub_elems : q_elems;
    bool sq = q_elems > 0;
    size_t n_cand = 0;
    for (size_t li = 0; sq && li < ops.size(); ++li) {
        const costa_tile_op_t& op = ops[li];
        if (op.nf <= 0 || op.ns <= 0 || !is_large(op, q_lo)) continue;
        ++n_cand;
        // c128 (r4): also lists whose large ops are aligned whole multiples of the square
        // sub-tile, which then run in destination-address order (below): BASELINE cfg 4's 128^2
        // blocks 16384^2 2.288 -> 2.119-2.134 ms, 32768^2 9.32 -> 9.05-9.10 ms; the 64 x 128
        // shape in that order 2.346 / 9.51, the square shape in hint order 2.237 / 9.52
        // (profiles/r4e/, r4f/)
        const bool whole_q = E == 16 && (op.flags & vec_both) == vec_both && op.nf % sh.bf_q == 0 &&
                             op.ns % sh.bs_q == 0;
        sq = kn.force_sq || (op.nf <= sh.bf_q && op.ns <= sh.bs_q) || whole_q;
    }
    sq = sq && n_cand > 0;
    const int64_t large_lo = sq ? q_lo : sub_elems;
    size_t n_med = 0;
    for (size_t li = 0; li < ops.size(); ++li) {
        const costa_tile_op_t& op = ops[li];
        if (op.nf <= 0 || op.ns <= 0) continue;
        const int64_t elems = int64_t(op.nf) * op.ns;
        const bool aligned = (op.flags & vec_both) == vec_both;
        if (is_large(op, large_lo))
            cls[li] = 0;
        else if (med_elems > 0 && aligned && 2 * elems >= med_elems && (op.flags & COSTA_TILE_TRANSPOSE))
            cls[li] = 1, ++n_med;
        else
            cls[li] = 2;
    }
    // the medium class on 32 x 32 sub-tiles (nb = 32 blocks): in a transposing list whose
    // aligned transposing ops outside the large class that hold at least half a 32 x 32 sub-tile
    // all fit one, and are at least kMinMediumOps many
    bool med_sq = tr_shape && sh.bf_s > 0;
    size_t n_msq = 0, n_exact = 0;
    const int64_t s_elems = int64_t(sh.bf_s) * sh.bs_s;
    for (size_t li = 0; med_sq && li < ops.size(); ++li) {
        const costa_tile_op_t& op = ops[li];
        if (cls[li] == 0 || cls[li] == 3 || (op.flags & vec_both) != vec_both || !(op.flags & COSTA_TILE_TRANSPOSE))
            continue;
        if (2 * int64_t(op.nf) * op.ns < s_elems) continue;
        if (op.nf > sh.bf_s || op.ns > sh.bs_s) med_sq = false;
        ++n_msq;
        n_exact += op.nf == sh.bf_s && op.ns == sh.bs_s;
    }
    // ... and at least 9 in 10 of them fill a sub-tile exactly (partly filled 32 x 32 sub-tiles lost
    // to the wavefront path: fp32 24^2 blocks 1.105 against 0.688 ms, c64 28^2 1.43 against 1.14;
    // profiles/r2e/s32/partial.log)
    med_sq = med_sq && n_msq >= kMinMediumOps && n_exact * 10 >= n_msq * 9;
    if (med_sq) {
        n_med = n_msq;
        for (size_t li = 0; li < ops.size(); ++li) {
            const costa_tile_op_t& op = ops[li];
            if (cls[li] == 0 || cls[li] == 3) continue;
            const bool m = (op.flags & vec_both) == vec_both && (op.flags & COSTA_TILE_TRANSPOSE) &&
                           2 * int64_t(op.nf) * op.ns >= s_elems;
            cls[li] = m ? 1 : 2;
        }
    }
    // transposes whose destination columns are off the 16-byte grid (an odd ScaLAPACK lld) go to
    // the skew shape (tile_kernels.hip skew_kernel): the cut between its sub-tiles follows the
    // 64-byte granules of each destination column, so no granule is shared by two workgroups
    // (measured: a copy whose 128-byte lines are split between workgroups at 16-byte granularity
    // 0.808 against 0.672 ms, at 64-byte granularity 0.702; tools/partial_line_probe.hip).  Every
    // element is written once: ops that read C (beta != 0) go there too.
    const int64_t k_elems = int64_t(sh.bf_k) * sh.bs_k;
    static const bool skew_on = [] {  // COSTA_SKEW=0: off (tuning)
        const char* s = tuning_env("COSTA_SKEW");
        return !s || std::atoi(s) != 0;
    }();
    // r4: also destinations on the 16-byte grid whose columns start off the 64-byte one (lld not
    // a multiple of 8 fp64 / 16 fp32 elements): the large shape's column segments then share
    // their edge granules with the neighbouring sub-tiles.  fp64 16384^2 'T' lld + 2 / + 4
    // 1.046 / 1.015 -> 0.855 / 0.837 ms, beta != 0 1.444 -> 1.244; fp32 lld + 4 / + 8 / + 24
    // 0.687 / 0.620 / 0.595 -> 0.466 / 0.482 / 0.466; aligned and 64-byte-aligned ld unchanged
    // (profiles/r4l/)
    // (r6) ...except transposes into a destination range a destination-block group may write: a
    // custom layout's own block buffer (leading dimension within a group's budget) is written by
    // its group in whole 16-byte vectors whatever its alignment, so such ops stay on the wavefront
    // path, where cblock_groups finds them; left out, their block's other ops fail the exactness
    // test too (cfg 5 'T': 45 skew ops broke 334 groups into 2 672 wavefront pieces)
    const bool groups_on = cblock_enabled(dtype, kind);
    const int64_t group_budget = cblock_max_elems(E) - (16 / E - 1);
    for (size_t li = 0; skew_on && k_elems > 0 && li < ops.size(); ++li) {
        const costa_tile_op_t& op = ops[li];
        if (cls[li] == 3 || !(op.flags & COSTA_TILE_TRANSPOSE)) continue;
        const bool off_granule = op.dst % 64 != 0 || (uint64_t(op.ldd) * uint64_t(E)) % 64 != 0;
        if ((op.flags & COSTA_TILE_VEC_DST) && !off_granule) continue;
        if (op.dst % uint64_t(E) != 0 || 2 * int64_t(op.nf) * op.ns < k_elems)
            continue;
        if (cls[li] == 1) --n_med;
        if (groups_on && op.ns <= op.ldd && op.ldd <= group_budget) {
            cls[li] = 2;
            continue;
        }
        cls[li] = 4;
    }
    mark(2);
    std::vector<uint32_t> shaped[3];  // [0] large, [1] medium, [2] skew
    std::vector<costa_tile_op_t> skew_ops;
    for (size_t li = 0; li < ops.size(); ++li) {
        const int c = cls[li] == 1 && n_med < kMinMediumOps ? 2 : cls[li];
        if (c < 2) shaped[c].push_back(uint32_t(li));
        else if (c == 2) wave_ops.push_back(&ops[li]);
        else if (c == 4) skew_ops.push_back(ops[li]);
    }
    // skew ops that continue each other in source and destination (the tiles of one local
    // matrix) become one op: a tile edge inside a destination column would otherwise be a
    // partial granule shared by two workgroups again
    merge_adjacent(skew_ops, E);
    for (size_t i = 0; i < skew_ops.size(); ++i) shaped[2].push_back(uint32_t(i));
    // 4-byte types reading sources off the 16-byte grid too: the wide skew variant, its
    // f-neighbours (which share the misaligned source runs' partial lines) grouped on one XCD
    bool skew_wide = false;
    for (const auto& op : skew_ops)
        skew_wide = skew_wide || (E == 4 && (op.src % 16 != 0 || (uint64_t(op.lds) * uint64_t(E)) % 16 != 0));
    const int64_t skew_group = kn.skew_xcd >= 0 ? kn.skew_xcd : skew_wide ? kSkewWideGroup : 0;
    // each shape's ops in hint order when every one carries a hint; lists whose shaped ops all
    // transpose 8-byte elements then take the sub-tiles in destination-address order (wave_knobs)
    int64_t n_work[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {
        const int bf = c == 2 ? (skew_wide ? sh.bf_kw : sh.bf_k) : c ? (med_sq ? sh.bf_s : sh.bf_m) : sq ? sh.bf_q : sh.bf;
        const int bs = c == 2 ? (skew_wide ? sh.bs_kw : sh.bs_k) : c ? (med_sq ? sh.bs_s : sh.bs_m) : sq ? sh.bs_q : sh.bs;
        const std::vector<uint32_t>& sel = shaped[c];
        const std::vector<costa_tile_op_t>& src_ops = c == 2 ? skew_ops : ops;
        std::vector<uint32_t> sperm(sel.size());
        for (size_t i = 0; i < sel.size(); ++i) sperm[i] = uint32_t(i);
        if (kn.large_sort >= 1 && !sel.empty()) {
            bool hints = true;
            for (uint32_t li : sel) hints = hints && src_ops[li].order != 0;
            if (hints)
                std::stable_sort(sperm.begin(), sperm.end(), [&](uint32_t x, uint32_t y) {
                    return src_ops[sel[x]].order < src_ops[sel[y]].order;
                });
        }
        const size_t op0 = ordered.size(), w0 = work.size();
        for (const uint32_t k : sperm) {
            const costa_tile_op_t& op = src_ops[sel[k]];
            const uint64_t i = ordered.size();
            if (i > 0xFFFFFFFFull) throw error(COSTA_ERR_ARG, "costa: too many tiles in one list");
            ordered.push_back(op);
            const uint64_t n = uint64_t((int64_t(op.nf) + bf - 1) / bf) * uint64_t((int64_t(op.ns) + bs - 1) / bs);
            if (n > 0xFFFFFFFFull) throw error(COSTA_ERR_ARG, "costa: tile too large");
            for (uint64_t q = 0; q < n; ++q) work.push_back((i << 32) | q);
        }
        bool by_address = kn.large_sort == 2 || dst_order;
        if (kn.large_sort == 3 && !dst_order) {
            by_address = (E == 4 || E == 8 || (E == 16 && c == 0 && sq)) && ordered.size() > op0;
            for (size_t i = op0; i < ordered.size(); ++i)
                by_address = by_address && (ordered[i].flags & COSTA_TILE_TRANSPOSE);
        }
        if (by_address && work.size() - w0 > 1) {
            // sub-tiles by the address of their first destination element (stable)
            std::vector<std::pair<uint64_t, uint64_t>> key(work.size() - w0);
            for (size_t x = 0; x < key.size(); ++x) {
                const uint64_t wx = work[w0 + x];
                const costa_tile_op_t& op = ordered[size_t(wx >> 32)];
                const uint64_t q = wx & 0xFFFFFFFFull, nbf = uint64_t((int64_t(op.nf) + bf - 1) / bf);
                const int64_t f0 = int64_t(q % nbf) * bf, s0 = int64_t(q / nbf) * bs;
                const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
                key[x] = {op.dst + uint64_t((tr ? f0 * op.ldd + s0 : s0 * op.ldd + f0) * E), wx};
            }
            // Destination columns taller than 128 KiB are walked in panels of 128 KiB of rows, each
            // panel band by band (r4): the sub-tiles in flight then cover 4 adjacent bands of a
            // panel instead of one band's full height, and read 4 KiB of each source column
            // instead of 1 KiB.  c128 'T' 32768^2 (512 KiB columns) 9.06-9.07 -> 8.66 ms; fp64
            // 32768^2 4.35 -> 4.27; 64 / 32 KiB panels lost (profiles/r4p/, r4q/).  Lists of
            // one destination stride only (the panel is cut from row / column positions).
            int64_t panel = kn.panel_rows;
            const int64_t ld0 = ordered[size_t(key[0].second >> 32)].ldd;
            bool one_ld = true;
            for (size_t i = op0; i < ordered.size() && one_ld; ++i) one_ld = ordered[i].ldd == ld0;
            // (c64, on its 128 x 128 sub-tiles, ran 1 % slower with them: 4.36 against 4.31 ms)
            if (panel == 0)
                panel = ld0 * E > kPanelBytes && dtype != COSTA_CFLOAT ? kPanelBytes / E : -1;
            // key = panel (16 bits) | column (24) | row in the panel (24): a panel of 2^24 rows or
            // more, a column index or a panel index past its field keeps the plain address order
            if (panel >= (int64_t(1) << 24)) panel = -1;
            if (panel > 0 && one_ld) {
                uint64_t lo = ~uint64_t(0), hi = 0;
                for (const auto& k : key) {
                    lo = std::min(lo, k.first);
                    hi = std::max(hi, k.first);
                }
                const uint64_t ld = uint64_t(ld0), last = (hi - lo) / uint64_t(E);
                const bool fits = last / ld < (uint64_t(1) << 24) && ld / uint64_t(panel) < (uint64_t(1) << 16);
                if (fits) {
                    for (auto& k : key) {
                        const uint64_t e = (k.first - lo) / uint64_t(E);
                        const uint64_t row = e % ld, col = e / ld;
                        k.first = ((row / uint64_t(panel)) << 48) | (col << 24) | (row % uint64_t(panel));
                    }
                }
            }
            sort_pairs_by_key(key);
            for (size_t x = 0; x < key.size(); ++x) work[w0 + x] = key[x].second;
        }
        if (c == 2 && skew_group > 1 && work.size() - w0 > 1) {
            // runs of F f-neighbours at one destination position, then run r of every 8 runs
            // spread to positions r, r + 8, ...: dispatch goes round-robin over the 8 XCDs
            const int64_t F = skew_group;
            std::vector<std::pair<uint64_t, uint64_t>> key(work.size() - w0);
            for (size_t x = 0; x < key.size(); ++x) {
                const uint64_t wx = work[w0 + x];
                const costa_tile_op_t& op = ordered[size_t(wx >> 32)];
                const uint64_t q = wx & 0xFFFFFFFFull, nbf = uint64_t((int64_t(op.nf) + bf - 1) / bf);
                const int64_t f0 = int64_t(q % nbf) * bf, s0 = int64_t(q / nbf) * bs;
                const int64_t fp = f0 / (bf * F) * (bf * F);
                key[x] = {((op.dst + uint64_t((fp * op.ldd + s0) * E)) << 6) | uint64_t((f0 - fp) / bf), wx};
            }
            std::sort(key.begin(), key.end());
            const size_t n = key.size(), blk = size_t(8 * F);
            for (size_t b = 0; b < n; b += blk) {
                const size_t m = std::min(blk, n - b);
                for (size_t x = 0; x < m; ++x) {
                    const size_t run = x / size_t(F), in = x % size_t(F);
                    const size_t to = m == blk ? in * 8 + run : x;
                    work[w0 + b + to] = key[b + x].second;
                }
            }
        }
        n_work[c] = int64_t(work.size() - w0);
    }
    lap(0);
    // destination-block groups out of the wavefront ops (after the skew items in `work`)
    int64_t cblock_lds = 0;
    int cb_map = cb_round_robin;
    const int64_t n_cblock = cblock_groups(dtype, wave_ops, kind, ordered, work, cblock_lds, cb_map, ops, dev);
    const size_t n_dev = dev ? dev->n_ordered : 0;  // the groups' entries left on the GPU
    lap(1);
    // ops are independent (disjoint destinations), so any order is valid; neighbours in
    // memory run at the same time and share the partially used cache lines at their edges.
    // The wavefront ops are ordered first, then cut into their pieces straight into the ordered
    // list (pieces of one op stay together, in f-major order).
    const size_t nw = wave_ops.size();
    uint32_t top = 0;  // largest hint (0: none of the ops carries one)
    bool tr = false;
    for (const auto* o : wave_ops) {
        top = std::max(top, o->order);
        tr = tr || (o->flags & COSTA_TILE_TRANSPOSE);
    }
    const int mode = kn.sort == 5   ? (pack_list ? 1 : 2)
                     : kn.sort == 4 ? (tr || top == 0 ? 2 : 3)
                     : kn.sort == 3 && top == 0 ? 2 : kn.sort;
    std::vector<uint32_t> perm(nw);
    if (mode == 3 && size_t(top) <= 4 * nw + 1024) {
        // the planner's hints are ranks within the list: a stable counting sort
        std::vector<uint32_t> at(size_t(top) + 2, 0);
        for (const auto* o : wave_ops) ++at[size_t(o->order) + 1];
        for (size_t k = 1; k < at.size(); ++k) at[k] += at[k - 1];
        for (size_t i = 0; i < nw; ++i) perm[at[wave_ops[i]->order]++] = uint32_t(i);
    } else if (mode == 2 && nw > 0) {
        // by destination address: a stable LSD radix sort of the element offsets from the lowest
        // destination (14-bit digits, only as many passes as the span needs)
        uint64_t lo = ~uint64_t(0), hi = 0;
        for (const auto* o : wave_ops) {
            lo = std::min(lo, o->dst);
            hi = std::max(hi, o->dst);
        }
        std::vector<uint64_t> key(nw), key2(nw);
        std::vector<uint32_t> idx2(nw);
        for (size_t i = 0; i < nw; ++i) {
            key[i] = (wave_ops[i]->dst - lo) / uint64_t(E);
            perm[i] = uint32_t(i);
        }
        const uint64_t span = (hi - lo) / uint64_t(E);
        constexpr int B = 14;
        std::vector<uint32_t> at((1 << B) + 1);
        for (int shift = 0; shift == 0 || (shift < 64 && (span >> shift) != 0); shift += B) {
            std::fill(at.begin(), at.end(), 0u);
            for (size_t i = 0; i < nw; ++i) ++at[((key[i] >> shift) & ((1 << B) - 1)) + 1];
            for (int d = 1; d <= (1 << B); ++d) at[d] += at[d - 1];
            for (size_t i = 0; i < nw; ++i) {
                const uint32_t p = at[(key[i] >> shift) & ((1 << B) - 1)]++;
                key2[p] = key[i];
                idx2[p] = perm[i];
            }
            key.swap(key2);
            perm.swap(idx2);
        }
    } else if (mode >= 1 && mode <= 3) {  // sort (key, index) pairs: stable
        std::vector<std::pair<uint64_t, uint32_t>> key(nw);
        for (size_t i = 0; i < nw; ++i) {
            const costa_tile_op_t& o = *wave_ops[i];
            key[i] = {mode == 1 ? o.src : mode == 2 ? o.dst : o.order, uint32_t(i)};
        }
        std::sort(key.begin(), key.end());
        for (size_t i = 0; i < nw; ++i) perm[i] = key[i].second;
    } else {
        for (size_t i = 0; i < nw; ++i) perm[i] = uint32_t(i);
    }
    if (kn.xcd_bands && mode == 2 && top > 0 && nw > 1) xcd_bands(wave_ops, E, kn.xcd_bands, local, perm);
    lap(2);
    // pieces: count per op, scan, fill (host threads for long lists)
    std::vector<wave_grid> grid(nw);
    std::vector<size_t> at_piece(nw + 1, 0);
    host_parallel(nw, [&](size_t b, size_t e) {
        for (size_t i = b; i < e; ++i) grid[i] = wave_pieces(*wave_ops[perm[i]], E, local);
    });
    for (size_t i = 0; i < nw; ++i)
        at_piece[i + 1] = at_piece[i] + size_t(grid[i].nfc * grid[i].nsc);
    work_split w;
    w.tr_shape = tr_shape;
    w.sq = sq;
    w.full = tr_shape && !sq && !shaped[0].empty();
    for (const uint32_t li : shaped[0]) {
        const costa_tile_op_t& op = ops[li];
        w.full = w.full && (op.flags & vec_both) == vec_both && op.nf % sh.bf == 0 && op.ns % sh.bs == 0;
    }
    w.med_sq = med_sq && !shaped[1].empty();
    w.med_full = !shaped[1].empty() && n_work[1] > 0 && !w.med_sq;
    for (const uint32_t li : shaped[1])
        w.med_full = w.med_full && ops[li].nf % sh.bf_m == 0 && ops[li].ns % sh.bs_m == 0;
    w.n_large = n_work[0];
    w.n_medium = n_work[1];
    w.n_skew = n_work[2];
    w.skew_wide = skew_wide && n_work[2] > 0;
    w.n_cblock = n_cblock;
    w.cblock_lds = cblock_lds;
    w.cb_map = cb_map;

    w.tiny_first = int64_t(ordered.size() + n_dev);
    w.n_tiny = int64_t(at_piece[nw]);
    const size_t base = ordered.size();
    ordered.resize(base + at_piece[nw]);
    host_parallel(nw, [&](size_t b, size_t e) {
        for (size_t i = b; i < e; ++i)
            emit_pieces(*wave_ops[perm[i]], E, grid[i], local, &ordered[base + at_piece[i]]);
    });
    if (trace) {
        lap(3);
        std::fprintf(stderr,
                     "[costa build_work] %zu ops (%s list): classify + shaped %.2f ms (merge %.2f, flags + "
                     "granules %.2f, classify %.2f, work items %.2f), groups %.2f (%lld), "
                     "wavefront order %.2f, pieces %.2f (%lld)\n",
                     ops_in.size(), pack_list ? "pack" : local ? "local" : "unpack", bw_t[0], sub_t[0],
                     sub_t[1] - sub_t[0], sub_t[2] - sub_t[1], bw_t[0] - sub_t[2], bw_t[1] - bw_t[0],
                     (long long)n_cblock, bw_t[2] - bw_t[1], bw_t[3] - bw_t[2], (long long)w.n_tiny);
    }
    return w;
}

launch_args make_launch(const work_split& w, const void* d_ordered, const void* d_work,
                        const char* src_base, char* dst_base, const void* d_scalars, bool transpose,
                        bool axpby) {
    launch_args a;
    a.ops = static_cast<const costa_tile_op_t*>(d_ordered);
    a.work = static_cast<const uint64_t*>(d_work);
    a.n_large = w.n_large;
    a.n_medium = w.n_medium;
    a.n_skew = w.n_skew;
    a.n_cblock = w.n_cblock;
    a.cblock_lds = w.cblock_lds;
    a.cb_map = w.cb_map;
    a.tiny_first = w.tiny_first;
    a.n_tiny = w.n_tiny;
    a.src_base = src_base;
    a.dst_base = dst_base;
    a.scalars = d_scalars;
    a.any_transpose = transpose;
    a.any_axpby = axpby;
    a.tr_shape = w.tr_shape;
    a.sq = w.sq;
    a.full = w.full;
    a.med_full = w.med_full;
    a.med_sq = w.med_sq;
    a.skew_wide = w.skew_wide;
    return a;
}

// ---------------------------------------------------------------- residency / staging
namespace {

// Byte ranges of host memory touched by a layout's blocks, merged; used to stage
// host-resident matrices through HBM (the path starts and ends in host memory).
struct hrange {
    uintptr_t lo, hi;
    size_t dev_off;
};

size_t block_extent_bytes(const eblock& b, char ordering, size_t E) {
    const int64_t nr = b.rows.length(), nc = b.cols.length();
    if (nr == 0 || nc == 0) return 0;
    const int64_t fast = ordering == 'R' ? nc : nr, slow = ordering == 'R' ? nr : nc;
    return size_t((slow - 1) * int64_t(b.ld) + fast) * E;
}

bool is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

// true if every block is in device memory; false if every block is host memory
bool layout_on_device(const elayout& L) {
    if (L.blocks.empty()) return true;
    bool first = is_device_ptr(L.blocks.front().data);
    // check block pointers that leave the current device allocation
    uintptr_t lo = 0, hi = 0;
    for (const auto& b : L.blocks) {
        uintptr_t p = reinterpret_cast<uintptr_t>(b.data);
        if (first && p >= lo && p < hi) continue;
        bool d = is_device_ptr(b.data);
        if (d != first)
            throw error(COSTA_ERR_ARG, "costa: a layout mixes host and device blocks");
        if (d) {
            hipDeviceptr_t base = nullptr;
            size_t sz = 0;
            if (hipMemGetAddressRange(&base, &sz, const_cast<char*>(b.data)) == hipSuccess) {
                lo = reinterpret_cast<uintptr_t>(base);
                hi = lo + sz;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    return first;
}

}  // namespace

// ---------------------------------------------------------------- host staging mode
namespace {
int g_host_mode = -1;
}
int host_staging_mode() {
    if (g_host_mode < 0) {
        const char* s = std::getenv("COSTA_HOST_STAGING");
        g_host_mode = s ? (std::atoi(s) != 0) : 1;
    }
    return g_host_mode;
}
void set_host_staging_mode(int mode) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    g_host_mode = mode != 0;
}

// ---------------------------------------------------------------- plan cache
namespace {

struct hasher {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    uint64_t h2 = 0x2545F4914F6CDD1Dull;  // second lane: other seed, other multiplier
    void mix(uint64_t v) {
        v ^= v >> 33;
        v *= 0xff51afd7ed558ccdull;
        v ^= v >> 33;
        h = (h ^ v) * 0xc4ceb9fe1a85ec53ull + 0x165667b19e3779f9ull;
        h ^= h >> 29;
        h2 = (h2 + v) * 0x9fb21c651e98df25ull;
        h2 ^= h2 >> 31;
    }
    void mix_vec(const std::vector<int>& v) {
        mix(v.size());
        for (int x : v) mix(uint64_t(uint32_t(x)));
    }
    void mix_layout(const elayout& L) {
        mix(uint64_t(L.dtype));
        mix(uint64_t(uint8_t(L.ordering)));
        mix(uint64_t(L.n_ranks));
        mix_vec(L.rows_split);
        mix_vec(L.cols_split);
        mix_vec(L.owners);
        mix(L.blocks.size());
        for (const auto& b : L.blocks) {
            mix(uint64_t(uint32_t(b.rows.start)) | (uint64_t(uint32_t(b.rows.end)) << 32));
            mix(uint64_t(uint32_t(b.cols.start)) | (uint64_t(uint32_t(b.cols.end)) << 32));
            mix(reinterpret_cast<uintptr_t>(b.data));
            mix(uint64_t(uint32_t(b.ld)));
        }
    }
};

}  // namespace

uint64_t layout_hash(const elayout& L) {
    hasher h;
    h.mix_layout(L);
    return h.h | 1;  // never 0 (0 = "not computed")
}

void layout_hashes(const elayout& L, uint64_t& h1, uint64_t& h2) {
    hasher h;
    h.mix_layout(L);
    h1 = h.h | 1;
    h2 = h.h2;
}

void set_layout_hash(elayout& L) { layout_hashes(L, L.hash, L.hash2); }

namespace {

// an uploaded op list with its work list
struct dev_list {
    dbuf ops, work;
    template <typename Op>
    const Op* list() const { return static_cast<const Op*>(ops.p); }
    const uint64_t* items() const { return static_cast<const uint64_t*>(work.p); }
};

// What one phase of a plan launches (LOCAL, one exchange round's PACK, one round's UNPACK), in launch
// order.  build_phase fills it, upload_phase brings the lists to the device, launch_phase runs them
// and count_phase keeps the statistics: a new list kind is a member here and a step in those four.
struct phase_lists {
    // the ordinary ops: tile_kernel lists (`split`: how the work list divides over the kernel shapes), or
    // the converting family's (`convert`) where the phase changes the element type -- LOCAL of a mixed
    // plan, PACK of a narrowing pair, UNPACK of a widening one; at most one of the two is non-empty
    dev_list tiles;
    work_split split;
    strip_list convert;
    bool transposes = false, reads_c = false;  // any op of `tiles` transposes / reads C
    // edge tiles of a triangular plan (tri_kernels.hip)
    dev_list tri;
    strip_list tri_items;
    // the ops of a scaled plan (scaled_kernels.hip, mx_kernels.hip, block_kernels.hip by the call's scheme)
    dev_list scaled;
    strip_list scaled_items;
    // the 128 x 128 regions of block_kernel's quantising form over scaled.ops (plans whose C holds FP8)
    dbuf block_work;
    strip_list block_items;
    // the dual ops of a dual-output MX plan (mx_dual_kernels.hip): the scaled ops with their twins in Ct,
    // in place of `scaled`
    dev_list dual;
    strip_list dual_items;
    bool empty() const {
        return !split.n_items() && !convert.n_items && !tri_items.n_items && !scaled_items.n_items &&
               !dual_items.n_items;
    }
};

struct cached_plan {
    std::unique_ptr<plan> p;
    int device = 0;
    // staging of host-resident layouts (empty when everything is in HBM)
    bool staged = false;
    std::vector<hrange> h2d_ranges, d2h_ranges;  // uploaded / copied back
    dbuf stage;
    phase_lists local;  // LOCAL
    dbuf d_scal;
    // the tile-boundary rule of MX calls per c_scales axis: 0 not checked yet, 1 holds, -1 fails
    int mx_rule[2] = {0, 0};
    // ... and of block-scaled FP8 calls per block shape of c_scales ((1,128), (128,1), (128,128))
    int blk_rule[3] = {0, 0, 0};
    // a dual-output MX plan (job::Ct): every LOCAL / UNPACK op with its twin, in the plan's order (the twin
    // rule held when they were built), and the block rule of both outputs per (c_scales, ct_scales) axis
    std::vector<costa_dual_op_t> local_dual, unpack_dual;
    int dual_rule[2][2] = {{0, 0}, {0, 0}};
    struct xround {  // one exchange round: its pack ops (by their first element) and unpack
                     // ops (by their last element)
        phase_lists pack, unpack;
    };
    std::vector<std::unique_ptr<xround>> rounds;
    std::vector<unsigned char> scal_host;
    std::shared_ptr<host_pipeline> pipe;  // host-resident single-rank calls (host_pipe.cpp)
};

constexpr size_t kMaxPlans = 16;
// A plan is found by a 64-bit hash and then verified against its full key: the second content
// hash of every layout plus cheap identity fields (sizes, first / last block pointer and ld).
// A hit on the hash alone would replay another layout pair's raw device addresses.
struct keyed_plan {
    uint64_t h = 0;
    std::vector<uint64_t> key;
    std::unique_ptr<cached_plan> plan;
};
std::list<keyed_plan> g_plans;  // MRU first

void key_layout(std::vector<uint64_t>& k, const elayout& L) {
    uint64_t h1 = L.hash, h2 = L.hash2;
    if (!h1) layout_hashes(L, h1, h2);  // C++-API layouts are hashed per call
    k.push_back(h1);
    k.push_back(h2);
    k.push_back(uint64_t(L.dtype) | uint64_t(uint8_t(L.ordering)) << 8 |
                uint64_t(uint32_t(L.n_ranks)) << 32);
    k.push_back(uint64_t(uint32_t(L.nbr())) | uint64_t(uint32_t(L.nbc())) << 32);
    k.push_back(L.blocks.size());
    if (!L.blocks.empty())
        for (const eblock* b : {&L.blocks.front(), &L.blocks.back()}) {
            k.push_back(reinterpret_cast<uintptr_t>(b->data));
            k.push_back(uint64_t(uint32_t(b->ld)) | uint64_t(uint32_t(b->rows.start)) << 32);
        }
}

// remap every block pointer of `L` that lies in a staged range to its device address
elayout remap(const elayout& L, const std::vector<hrange>& ranges, char* dev) {
    elayout out = L;
    for (auto& b : out.blocks) {
        uintptr_t p = reinterpret_cast<uintptr_t>(b.data);
        auto it = std::upper_bound(ranges.begin(), ranges.end(), p,
                                   [](uintptr_t v, const hrange& r) { return v < r.lo; });
        if (it == ranges.begin()) throw error(COSTA_ERR_INTERNAL, "costa: staging map miss");
        --it;
        b.data = dev + it->dev_off + (p - it->lo);
    }
    return out;
}

std::vector<hrange> collect_ranges(const std::vector<const elayout*>& Ls) {
    std::vector<hrange> r;
    for (const elayout* L : Ls) {
        const size_t E = dtype_size(L->dtype);
        for (const auto& b : L->blocks) {
            size_t ext = block_extent_bytes(b, L->ordering, E);
            if (!ext) continue;
            uintptr_t lo = reinterpret_cast<uintptr_t>(b.data);
            r.push_back({lo, lo + ext, 0});
        }
    }
    std::sort(r.begin(), r.end(), [](const hrange& x, const hrange& y) { return x.lo < y.lo; });
    std::vector<hrange> m;
    for (const auto& x : r) {
        if (!m.empty() && x.lo <= m.back().hi)
            m.back().hi = std::max(m.back().hi, x.hi);
        else
            m.push_back(x);
    }
    return m;
}

}  // namespace

// ---------------------------------------------------------------- planner choice
namespace {
int g_planner = -1;                         // costa_hip_set_planner / COSTA_PLANNER
constexpr size_t kDevicePlanBlocks = 4096;  // smaller layout pairs plan on the host
// The first GPU plan of a process loads the planner's kernels (about 15 ms on MI355X); before
// that, only layout pairs whose host planning costs as much go to the GPU.
constexpr size_t kColdDevicePlanBlocks = 100000;
bool g_device_planner_warm = false;
}  // namespace

int planner_mode() {
    if (g_planner < 0) {
        const char* s = std::getenv("COSTA_PLANNER");
        g_planner = s ? std::max(0, std::min(2, std::atoi(s))) : 1;
    }
    return g_planner;
}

void set_planner_mode(int mode) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    g_planner = mode;
}

namespace {
int g_list_builder = -1;  // costa_hip_set_list_builder / COSTA_LIST_BUILDER
}  // namespace

int list_builder_mode() {
    if (g_list_builder < 0) {
        const char* s = std::getenv("COSTA_LIST_BUILDER");
        g_list_builder = s ? std::max(0, std::min(2, std::atoi(s))) : 1;
    }
    return g_list_builder;
}

void set_list_builder_mode(int mode) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    g_list_builder = mode;
}

namespace {
// a work list into device memory: the host entries around the section the GPU built
template <typename X>
void upload_list(dbuf& d, const std::vector<X>& h, const X* sec, size_t at, size_t n, hipStream_t s) {
    if (!sec || n == 0) return d.upload(h, s);
    const size_t total = h.size() + n;
    d.reserve(total * sizeof(X));
    X* p = static_cast<X*>(d.p);
    if (at) HIP_CHECK(hipMemcpyAsync(p, h.data(), at * sizeof(X), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(p + at, sec, n * sizeof(X), hipMemcpyDeviceToDevice, s));
    if (h.size() > at)
        HIP_CHECK(hipMemcpyAsync(p + at + n, h.data() + at, (h.size() - at) * sizeof(X), hipMemcpyHostToDevice, s));
}
}  // namespace

bool work_export(costa_dtype_t dtype, const std::vector<costa_tile_op_t>& ops, list_kind kind, int device,
                 std::vector<costa_tile_op_t>& ordered, std::vector<uint64_t>& work, work_split& w) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (device < 0) {
        w = build_work(dtype, ops, ordered, work, kind);
        return false;
    }
    device_ctx& dc = ctx(device);
    device_section sec;
    sec.device = device;
    sec.stream = dc.main;
    sec.force = true;
    w = build_work(dtype, ops, ordered, work, kind, &sec);
    if (!sec.n_ordered) return false;
    std::vector<costa_tile_op_t> o(sec.n_ordered);
    std::vector<uint64_t> k(sec.n_work);
    HIP_CHECK(hipMemcpyAsync(o.data(), sec.d_ordered, o.size() * sizeof(o[0]), hipMemcpyDeviceToHost, dc.main));
    HIP_CHECK(hipMemcpyAsync(k.data(), sec.d_work, k.size() * sizeof(k[0]), hipMemcpyDeviceToHost, dc.main));
    HIP_CHECK(hipStreamSynchronize(dc.main));
    ordered.insert(ordered.begin() + std::ptrdiff_t(sec.at_ordered), o.begin(), o.end());
    work.insert(work.begin() + std::ptrdiff_t(sec.at_work), k.begin(), k.end());
    return true;
}

namespace {
// the plan of a cache miss, built on the GPU when the planner mode asks for it and the layouts
// allow it (make_plan_device), else on the host; both give the same plan
std::unique_ptr<plan> plan_jobs(const std::vector<job>& jobs, comm* c, hipStream_t s) {
    const int lb = c->size == 1 && c->nccl ? loopback_exchange() : 0;
    const int mode = planner_mode();
    size_t blocks = 0;
    for (const job& j : jobs) blocks += j.A->blocks.size() + j.C->blocks.size();
    const size_t need = g_device_planner_warm ? kDevicePlanBlocks : kColdDevicePlanBlocks;
    // (FP4 and FP6 pairs are planned on the host, whatever the mode: make_plan holds their evenness /
    // quad rule)
    if (!any_packed(jobs) && (mode == 2 || (mode == 1 && blocks >= need))) {
        if (auto p = make_plan_device(jobs, c->rank, c->size, lb, c->device, s)) {
            g_stats.device_plans++;
            g_device_planner_warm = true;
            return p;
        }
    }
    return make_plan(jobs, c->rank, c->size, lb);
}

// the element types a converting plan's PACK list runs on: a packed FP4 / FP6 package is copied as
// bytes by the FP8 family's Q -> Q kernel (scale kind BITCOPY: the bits of every byte)
costa_dtype_t pack_src(const plan& p) { return dtype_is_packed(p.src_dtype) ? COSTA_FP8_E4M3 : p.src_dtype; }
costa_dtype_t pack_dst(const plan& p) { return dtype_is_packed(p.pkg_dtype) ? COSTA_FP8_E4M3 : p.pkg_dtype; }

// the element types a phase reads and writes (its tile_kernel, edge-tile and same-type lists run on dst)
struct dtype_pair {
    costa_dtype_t src, dst;
};
dtype_pair phase_dtypes(const plan& p, list_kind kind) {
    if (kind == list_pack) return {pack_src(p), pack_dst(p)};
    return {kind == list_unpack ? p.pkg_dtype : p.src_dtype, p.dtype};
}

// The kernels a phase's ordinary ops run on.
// (a mixed plan's LOCAL list converts; its package holds the narrower type, so PACK converts
// for narrowing pairs and UNPACK for widening ones, the other being a same-type list; every
// list of a half-precision plan runs on the converting family, its same-type H -> H lists too)
// (an FP8 plan's package holds A's type: PACK is a byte copy on the FP8 family when A holds Q and
// an ordinary FLOAT list when A is FLOAT; UNPACK always runs on the FP8 family, Q -> Q included)
// (an FP4 / FP6 plan is a scaled plan, its ordinary LOCAL and UNPACK lists are empty; PACK is a byte
// copy on the FP8 family when A holds the packed type -- pack_src / pack_dst -- and a FLOAT list
// when A is FLOAT)
enum class tiles_on { none, tile_kernel, converting };
tiles_on phase_tiles(const plan& p, list_kind kind) {
    bool cv;
    if (kind == list_pack)
        cv = p.half() || (p.packed() ? dtype_is_packed(p.src_dtype)
                          : p.fp8()  ? dtype_is_fp8(p.src_dtype)
                                     : p.mixed() && p.pkg_dtype != p.src_dtype);
    else if (p.packed())
        return tiles_on::none;
    else if (kind == list_local)
        cv = p.converting();
    else
        cv = p.half() || p.fp8() || (p.mixed() && p.pkg_dtype != p.dtype);
    return cv ? tiles_on::converting : tiles_on::tile_kernel;
}

// a phase's lists in host memory, between build_phase and upload_phase (`into`: where they go)
struct host_lists {
    phase_lists* into;
    std::vector<costa_tile_op_t> tiles;
    std::vector<costa_tri_op_t> tri;
    std::vector<costa_scaled_op_t> scaled;
    std::vector<costa_dual_op_t> dual;
    std::vector<uint64_t> tiles_work, tri_work, scaled_work, block_work, dual_work;
    // the destination-block groups of long lists are built on the GPU and stay there
    device_section sec;
    host_lists(phase_lists& ph, int device, hipStream_t s) : into(&ph) {
        sec.device = device;
        sec.stream = s;
    }
};

// One phase's lists from its ops (package offsets are relative to the 256-byte aligned send / receive
// buffers): the counts and flags into *h.into, the lists into h.
void build_phase(const plan& p, list_kind kind, bool masked, const std::vector<costa_tile_op_t>& tiles,
                 const std::vector<costa_tri_op_t>& tri, const std::vector<costa_scaled_op_t>& scaled,
                 host_lists& h, const std::vector<costa_dual_op_t>* dual = nullptr) {
    phase_lists& ph = *h.into;
    const dtype_pair t = phase_dtypes(p, kind);
    // (a pack list is launched as one that neither transposes nor reads C)
    ph.transposes = kind != list_pack && any_transpose(tiles);
    ph.reads_c = kind != list_pack && any_axpby(tiles);
    switch (phase_tiles(p, kind)) {
    case tiles_on::converting:
        ph.convert = build_convert_work(t.src, t.dst, tiles, 0, 0, h.tiles, h.tiles_work);
        break;
    case tiles_on::tile_kernel:
        // The wholly kept tiles of a triangular plan merge into row bands of unequal widths, one
        // sub-tile tall: in list order consecutive workgroups walk along a band, a sub-tile's
        // columns apart, and a copy list ran at 3.8 TB/s against 6.7 for the full rectangle;
        // in destination-address order 6.2 (16384^2 fp64 'N').
        ph.split = build_work(t.dst, tiles, h.tiles, h.tiles_work, kind, kind == list_pack ? nullptr : &h.sec,
                              kind == list_local && masked);
        break;
    case tiles_on::none:
        break;
    }
    if (!tri.empty()) ph.tri_items = build_tri_work(t.dst, tri, 0, 0, h.tri, h.tri_work);
    if (scaled.empty()) return;
    // a scaled plan's LOCAL list, its sub-tiles in destination-address order (COSTA_SCALED_ORDER=0,
    // tuning: list order; DESIGN 3h has both)
    static const bool local_by_dst = [] {
        const char* e = tuning_env("COSTA_SCALED_ORDER");
        return !e || std::atoi(e) != 0;
    }();
    const bool by_dst = kind == list_local && local_by_dst;
    if (dual) {  // a dual-output MX plan: the same ops with their twins, on mx_dual_kernel alone
        ph.dual_items = build_dual_work(t.dst, *dual, 0, 0, 0, h.dual, h.dual_work, by_dst);
        return;
    }
    ph.scaled_items = build_scaled_work(t.src, t.dst, scaled, 0, 0, h.scaled, h.scaled_work, by_dst);
    // (a scaled plan into FP8 also serves block-scaled calls: the regions of its quantising kernel)
    if (block_pair(p.src_dtype, p.dtype) && dtype_is_fp8(p.dtype)) {
        std::vector<costa_scaled_op_t> same;  // (the ops of h.scaled)
        ph.block_items = build_block_work(t.src, t.dst, scaled, 0, 0, same, h.block_work, by_dst);
    }
}

void upload_phase(const host_lists& h, hipStream_t s) {
    phase_lists& ph = *h.into;
    upload_list(ph.tiles.ops, h.tiles, h.sec.d_ordered, h.sec.at_ordered, h.sec.n_ordered, s);
    upload_list(ph.tiles.work, h.tiles_work, h.sec.d_work, h.sec.at_work, h.sec.n_work, s);
    if (ph.tri_items.n_items) {
        ph.tri.ops.upload(h.tri, s);
        ph.tri.work.upload(h.tri_work, s);
    }
    if (ph.scaled_items.n_items) {
        ph.scaled.ops.upload(h.scaled, s);
        ph.scaled.work.upload(h.scaled_work, s);
    }
    if (ph.block_items.n_items) ph.block_work.upload(h.block_work, s);
    if (ph.dual_items.n_items) {
        ph.dual.ops.upload(h.dual, s);
        ph.dual.work.upload(h.dual_work, s);
    }
}

// the ops of each of R exchange rounds, in list order
template <typename Op>
std::vector<std::vector<Op>> by_round(const std::vector<Op>& ops, const std::vector<int>& round, int R) {
    std::vector<std::vector<Op>> out(static_cast<size_t>(R));
    for (size_t i = 0; i < ops.size(); ++i) out[size_t(round[i])].push_back(ops[i]);
    return out;
}

// Every phase of cp's plan: LOCAL, and PACK and UNPACK of each exchange round.  Pack ops go to the
// round of their first element (every element a round sends is packed by then), unpack ops to the
// round of their last (every element they read has arrived).
std::vector<host_lists> build_lists(cached_plan& cp, comm* c, hipStream_t s, bool masked,
                                    const elayout* Ct = nullptr) {
    const plan& p = *cp.p;
    if (Ct) {  // a dual-output MX plan: the twin of every scaled op, or the "dual layouts" error
        cp.local_dual = dual_twins(p.local_scaled, *Ct, p.rank);
        cp.unpack_dual = dual_twins(p.unpack_scaled, *Ct, p.rank);
        check_dual_ops(p.dtype, cp.local_dual, -1, -1, 0, 0);  // (the packed rules on Ct's side)
        check_dual_ops(p.dtype, cp.unpack_dual, -1, -1, 0, 0);
    }
    if (p.packed() && (!p.local_ops.empty() || !p.unpack_ops.empty()))
        throw error(COSTA_ERR_INTERNAL, "costa: an FP4 / FP6 plan with ordinary LOCAL / UNPACK ops");
    const int R = c->exchanges() ? exchange_rounds() : 1;
    std::vector<int> pr, ur, tr, sr;
    exchange_round_of_ops(p, R, pr, ur);
    exchange_round_of_tri(p, R, tr);
    exchange_round_of_scaled(p, R, sr);
    const auto pack = by_round(p.pack_ops, pr, R), unpack = by_round(p.unpack_ops, ur, R);
    const auto unpack_tri = by_round(p.unpack_tri, tr, R);
    const auto unpack_scaled = by_round(p.unpack_scaled, sr, R);
    std::vector<std::vector<costa_dual_op_t>> unpack_dual;
    if (Ct) unpack_dual = by_round(cp.unpack_dual, sr, R);
    std::vector<host_lists> h;
    h.reserve(1 + 2 * size_t(R));
    h.emplace_back(cp.local, cp.device, s);
    build_phase(p, list_local, masked, p.local_ops, p.local_tri, p.local_scaled, h.back(),
                Ct ? &cp.local_dual : nullptr);
    for (size_t r = 0; r < size_t(R); ++r) {
        cp.rounds.push_back(std::make_unique<cached_plan::xround>());
        h.emplace_back(cp.rounds.back()->pack, cp.device, s);
        build_phase(p, list_pack, false, pack[r], {}, {}, h.back());
        h.emplace_back(cp.rounds.back()->unpack, cp.device, s);
        build_phase(p, list_unpack, false, unpack[r], unpack_tri[r], unpack_scaled[r], h.back(),
                    Ct ? &unpack_dual[r] : nullptr);
    }
    return h;
}

std::vector<uint64_t> plan_key(const std::vector<job>& jobs, const comm* c) {
    std::vector<uint64_t> key;
    key.reserve(4 + jobs.size() * 30);
    key.push_back(uint64_t(uint32_t(c->rank)) | uint64_t(uint32_t(c->size)) << 32);
    key.push_back(uint64_t(uint32_t(c->device)) | uint64_t(uint32_t(host_staging_mode())) << 32);
    key.push_back(jobs.size());
    for (const auto& j : jobs) {
        key_layout(key, *j.A);  // handles cache their hashes
        key_layout(key, *j.C);
        uint64_t w = uint64_t(uint8_t(std::toupper(static_cast<unsigned char>(j.trans))));
        // the scale kinds (not the values) are baked into the ops
        for (bool cm : {true, false})
            w = w << 8 | scale_kind(j.C->dtype, j.s, cm, std::toupper(j.trans) == 'C');
        key.push_back(w);
        // the mask of a triangular transform
        // ... and whether the ops carry target coordinates (a scaled transform; its vectors are
        // arguments of the call, not of the plan)
        key.push_back(uint64_t(uint8_t(std::toupper(static_cast<unsigned char>(j.uplo)))) << 32 |
                      uint64_t(j.scaled) << 40 | uint64_t(j.Ct != nullptr) << 41 | uint64_t(uint32_t(j.k)));
        // a dual-output MX call: its lists hold Ct's addresses
        if (j.Ct) key_layout(key, *j.Ct);
    }
    return key;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// why a batch takes device-resident layouts only, or nullptr
const char* device_only(const std::vector<job>& jobs) {
    const bool packed = any_packed(jobs);
    if (packed && (dtype_is_fp6(jobs[0].A->dtype) || dtype_is_fp6(jobs[0].C->dtype)))
        return "costa: FP6 transforms (A or C of a packed 6-bit element type) need "
               "device-resident layouts";
    if (packed)
        return "costa: FP4 transforms (A or C of the packed 4-bit element type) need "
               "device-resident layouts";
    if (any_fp8(jobs))  // 1-byte element types: treated like mixed pairs here
        return "costa: FP8 transforms (A or C of a 1-byte element type) need "
               "device-resident layouts";
    if (any_half(jobs))  // 2-byte element types: the same
        return "costa: half-precision transforms (A or C of a 2-byte element type) need "
               "device-resident layouts";
    if (any_mixed(jobs))
        return "costa: mixed-precision transforms (A and C of different element types) need "
               "device-resident layouts";
    if (any_scaled(jobs)) return "costa: scaled transforms need device-resident layouts";
    return nullptr;
}

// the host-resident layouts of a batch, staged in cp.stage: the jobs on their device copies
struct staging {
    std::vector<job> jobs;
    std::vector<elayout> remapped;
    std::vector<hrange> ranges;
    // per merged range: holds A data (bit 0), C data (bit 1), C blocks of more than one
    // job (bit 2); C ranges are copied back, A ranges and C ranges the kernels do not
    // overwrite completely are uploaded (decided once the ops are known: staged_copies)
    std::vector<uint8_t> flags;
};

// Residency: all device, or stage the host-resident layouts (cp.staged, cp.stage, st).  -> true when
// the batch takes the pipelined scheme instead (host_pipe.cpp): cp is then complete.
bool stage_host_layouts(const std::vector<job>& jobs, comm* c, device_ctx& dc, bool masked, cached_plan& cp,
                        staging& st) {
    bool all_dev = true;
    std::vector<bool> on_dev;
    for (const auto& j : jobs)
        for (const elayout* L : {j.A, j.C}) {
            bool d = layout_on_device(*L);
            on_dev.push_back(d);
            all_dev = all_dev && d;
        }
    st.jobs = jobs;
    if (all_dev) return false;
    if (const char* why = device_only(jobs)) throw error(COSTA_ERR_ARG, why);
    cp.staged = true;
    std::vector<const elayout*> As, Cs;
    size_t k = 0;
    for (const auto& j : jobs) {
        if (!on_dev[k++]) As.push_back(j.A);
        if (!on_dev[k++]) Cs.push_back(j.C);
    }
    std::vector<const elayout*> all = As;
    all.insert(all.end(), Cs.begin(), Cs.end());
    auto ranges = collect_ranges(all);
    size_t off = 0;
    for (auto& r : ranges) {
        r.dev_off = off;
        off += ((r.hi - r.lo) + 255) & ~size_t(255);
    }
    st.flags.assign(ranges.size(), 0);
    std::vector<int> c_job(ranges.size(), -1);
    auto range_of = [&](uintptr_t p) {
        auto it = std::upper_bound(ranges.begin(), ranges.end(), p,
                                   [](uintptr_t v, const hrange& r) { return v < r.lo; });
        return size_t(it - ranges.begin()) - 1;
    };
    k = 0;
    for (size_t t = 0; t < jobs.size(); ++t) {
        const bool a_host = !on_dev[k++], c_host = !on_dev[k++];
        for (int side = 0; side < 2; ++side) {
            if (!(side == 0 ? a_host : c_host)) continue;
            const elayout* L = side == 0 ? jobs[t].A : jobs[t].C;
            const size_t E = dtype_size(L->dtype);
            for (const auto& b : L->blocks) {
                if (!block_extent_bytes(b, L->ordering, E)) continue;
                const size_t i = range_of(reinterpret_cast<uintptr_t>(b.data));
                if (side == 0) {
                    st.flags[i] |= 1;
                } else {
                    st.flags[i] |= 2;
                    if (c_job[i] >= 0 && c_job[i] != int(t)) st.flags[i] |= 4;
                    c_job[i] = int(t);
                }
            }
        }
    }
    // Pipelined staging (host_pipe.cpp) when every layout is host-resident, no range holds
    // both source and target data (in-place) and no target range is shared by two jobs
    // (their updates would have to be applied in order).
    // (triangular transforms always take the mirror scheme)
    bool pipe_ok = host_staging_mode() == 1 && !masked &&
                   std::none_of(on_dev.begin(), on_dev.end(), [](bool d) { return d; });
    for (uint8_t f : st.flags)
        if ((f & 3) == 3 || (f & 4)) pipe_ok = false;
    if (pipe_ok) {
        const double tp = now_ms();
        auto hplan = plan_jobs(jobs, c, dc.main);  // host addresses
        g_stats.plan_ms += now_ms() - tp;
        if (host_pipeline_accepts(hplan->dtype, hplan->pack_ops)) {
            cp.staged = false;
            cp.p = std::move(hplan);
            const int R = c->exchanges() ? exchange_rounds() : 1;
            std::vector<int> pr, ur;
            exchange_round_of_ops(*cp.p, R, pr, ur);
            cp.pipe = make_host_pipeline(cp.p->dtype, cp.p->pack_ops, cp.p->local_ops,
                                         cp.p->unpack_ops, pr, ur, R);
            return true;
        }
    }
    cp.stage.reserve(std::max<size_t>(off, 256));
    st.remapped.reserve(jobs.size() * 2);
    k = 0;
    for (auto& j : st.jobs) {
        if (!on_dev[k++]) {
            st.remapped.push_back(remap(*j.A, ranges, static_cast<char*>(cp.stage.p)));
            j.A = &st.remapped.back();
        }
        if (!on_dev[k++]) {
            st.remapped.push_back(remap(*j.C, ranges, static_cast<char*>(cp.stage.p)));
            j.C = &st.remapped.back();
        }
    }
    st.ranges = std::move(ranges);
    return false;
}

// The copies of a staged plan: C ranges come back (d2h_ranges); A ranges go up, and C ranges unless
// the kernels overwrite every byte of them (h2d_ranges): one job's C blocks only, no op reading C
// (beta = 0), and the ops' writes (disjoint: each C element is written once per job) add up to the
// whole range.
void staged_copies(cached_plan& cp, const staging& st, bool masked) {
    const plan& p = *cp.p;
    const size_t E = dtype_size(p.dtype);
    const uintptr_t base = reinterpret_cast<uintptr_t>(cp.stage.p);
    std::vector<size_t> written(st.ranges.size(), 0);
    std::vector<bool> reads_c(st.ranges.size(), false);
    auto account = [&](const std::vector<costa_tile_op_t>& ops) {
        for (const auto& op : ops) {
            if (op.dst < base) continue;  // device-resident destination
            const size_t off = size_t(op.dst - base);
            auto it = std::upper_bound(st.ranges.begin(), st.ranges.end(), off,
                                       [](size_t v, const hrange& r) { return v < r.dev_off; });
            if (it == st.ranges.begin()) continue;
            const size_t i = size_t(it - st.ranges.begin()) - 1;
            if (off >= st.ranges[i].dev_off + (st.ranges[i].hi - st.ranges[i].lo)) continue;
            written[i] += size_t(op.nf) * size_t(op.ns) * E;
            if (((op.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT) == COSTA_SCALE_AXPBY)
                reads_c[i] = true;
        }
    };
    account(p.local_ops);
    account(p.unpack_ops);
    for (size_t i = 0; i < st.ranges.size(); ++i) {
        const hrange& r = st.ranges[i];
        const uint8_t f = st.flags[i];
        // (a masked plan never overwrites a range completely: dropped elements keep their bytes)
        const bool overwritten = !masked && f == 2 && !reads_c[i] && written[i] == r.hi - r.lo;
        if ((f & 1) || ((f & 2) && !overwritten)) cp.h2d_ranges.push_back(r);
        if (f & 2) cp.d2h_ranges.push_back(r);
    }
}

// a plan-cache miss: residency, the plan, its lists, their upload
std::unique_ptr<cached_plan> build_cached_plan(const std::vector<job>& jobs, comm* c, device_ctx& dc) {
    // COSTA_PLAN_TRACE=1: where a plan-cache miss spends its host time (stderr)
    static const bool trace = std::getenv("COSTA_PLAN_TRACE") != nullptr;
    const double t0 = now_ms();
    const bool masked = any_masked(jobs);
    if (masked || device_only(jobs)) {  // an unsupported pair is reported as such, whatever the residency
        costa_dtype_t a, b;
        check_jobs(jobs, c->size, a, b);
    }
    auto cp = std::make_unique<cached_plan>();
    cp->device = c->device;
    staging st;
    if (stage_host_layouts(jobs, c, dc, masked, *cp, st)) return cp;
    const double t_resid = now_ms() - t0;
    cp->p = plan_jobs(st.jobs, c, dc.main);
    const double t_plan = now_ms() - t0 - t_resid;
    g_stats.plan_ms += t_plan;
    if (cp->staged) staged_copies(*cp, st, masked);
    const std::vector<host_lists> lists = build_lists(*cp, c, dc.main, masked, st.jobs[0].Ct);
    const double t_work = now_ms() - t0 - t_resid - t_plan;
    for (const host_lists& h : lists) upload_phase(h, dc.main);
    HIP_CHECK(hipStreamSynchronize(dc.main));  // the host lists are temporaries
    if (trace)
        std::fprintf(stderr,
                     "[costa plan] %zu local / %zu pack / %zu unpack ops: residency %.2f ms, "
                     "planning %.2f, work lists %.2f, upload %.2f, total %.2f\n",
                     cp->p->local_ops.size(), cp->p->pack_ops.size(), cp->p->unpack_ops.size(), t_resid, t_plan,
                     t_work, now_ms() - t0 - t_resid - t_plan - t_work, now_ms() - t0);
    return cp;
}

cached_plan* get_plan(const std::vector<job>& jobs, comm* c, device_ctx& dc) {
    std::vector<uint64_t> key = plan_key(jobs, c);
    hasher h;
    for (uint64_t w : key) h.mix(w);
    for (auto it = g_plans.begin(); it != g_plans.end(); ++it) {
        if (it->h == h.h && it->key == key) {
            g_plans.splice(g_plans.begin(), g_plans, it);
            g_stats.plan_hits++;
            return g_plans.front().plan.get();
        }
    }
    g_stats.plan_misses++;
    auto cp = build_cached_plan(jobs, c, dc);
    g_plans.push_front({h.h, std::move(key), std::move(cp)});
    while (g_plans.size() > kMaxPlans) g_plans.pop_back();
    return g_plans.front().plan.get();
}

void upload_scalars(cached_plan& cp, const std::vector<job>& jobs, hipStream_t s) {
    const size_t E = dtype_size(cp.p->scalar_dtype());  // (fp32 for half-precision plans)
    std::vector<unsigned char> host(jobs.size() * 2 * E);
    for (size_t t = 0; t < jobs.size(); ++t) {
        std::memcpy(&host[(2 * t) * E], jobs[t].s.alpha.data(), E);
        std::memcpy(&host[(2 * t + 1) * E], jobs[t].s.beta.data(), E);
    }
    if (host != cp.scal_host || !cp.d_scal.p) {
        // stream-ordered behind earlier (possibly asynchronous) transforms that still read the
        // old values; pageable source -> the runtime stages it before returning
        cp.d_scal.reserve(host.size());
        cp.scal_host = host;
        HIP_CHECK(hipMemcpyAsync(cp.d_scal.p, cp.scal_host.data(), host.size(),
                                 hipMemcpyHostToDevice, s));
    }
}

}  // namespace

void release_caches() {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    g_plans.clear();
    release_host_rings();
    ctx_map().clear();
}

// ---------------------------------------------------------------- transform
// Phases are bracketed by pooled event pairs on the stream they run on; the pairs are
// resolved (elapsed time added to the statistics) at the next synchronisation point, so
// asynchronous transforms are timed too.
namespace {
// (PH_TRI_*: the edge-tile launches of triangular plans; their time counts as LOCAL / UNPACK time
// and is also kept on its own, tri_phase_ms())
enum phase { PH_LOCAL, PH_PACK, PH_EXCHANGE, PH_UNPACK, PH_H2D, PH_D2H, PH_TRI_LOCAL, PH_TRI_UNPACK };
double g_tri_ms = 0;
int64_t g_scaled_items = 0;  // sub-tiles run by scaled_kernel (kept beside costa_stats_t)
int64_t g_amax_items = 0;    // ... by its AMAX instantiations and by amax_kernel (likewise)
int64_t g_mx_items = 0;      // ... by mx_kernel (likewise; not counted as scaled items)
int64_t g_blk_items = 0;     // sub-tiles and regions run by block_kernel (likewise)
int64_t g_mx_dual_items = 0; // sub-tiles run by mx_dual_kernel (likewise; not counted as MX items)

struct phase_timer {
    device_ctx& dc;
    bool on;
    int ph = 0;
    hipEvent_t a = nullptr;
    hipStream_t s = nullptr;
    phase_timer(device_ctx& d, bool prof) : dc(d), on(prof) {}
    void start(int p, hipStream_t st) {
        if (!on) return;
        ph = p;
        s = st;
        a = dc.take_event();
        HIP_CHECK(hipEventRecord(a, s));
    }
    void stop() {
        if (!on || !a) return;
        hipEvent_t b = dc.take_event();
        HIP_CHECK(hipEventRecord(b, s));
        dc.pending.push_back({ph, a, b});
        a = nullptr;
        if (dc.pending.size() > 1024) dc.resolve(64);
    }
};
}  // namespace

void device_ctx::resolve(size_t max_n) {
    size_t n = 0;
    while (!pending.empty() && n < max_n) {
        timed t = pending.front();
        pending.pop_front();
        float ms = 0.f;
        HIP_CHECK(hipEventSynchronize(t.b));
        HIP_CHECK(hipEventElapsedTime(&ms, t.a, t.b));
        double* acc[] = {&g_stats.local_ms, &g_stats.pack_ms, &g_stats.exchange_ms,
                         &g_stats.unpack_ms, &g_stats.h2d_ms, &g_stats.d2h_ms};
        if (t.phase == PH_TRI_LOCAL || t.phase == PH_TRI_UNPACK) {
            (t.phase == PH_TRI_LOCAL ? g_stats.local_ms : g_stats.unpack_ms) += ms;
            g_tri_ms += ms;
        } else {
            *acc[t.phase] += ms;
        }
        free_events.push_back(t.a);
        free_events.push_back(t.b);
        ++n;
    }
}

hipEvent_t device_ctx::take_event() {
    if (free_events.empty()) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        return e;
    }
    hipEvent_t e = free_events.back();
    free_events.pop_back();
    return e;
}

void resolve_pending() {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    for (auto& kv : ctx_map()) {
        HIP_CHECK(hipSetDevice(kv.first));
        kv.second->resolve();
    }
}

double tri_phase_ms(bool reset) {
    resolve_pending();
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const double v = g_tri_ms;
    if (reset) g_tri_ms = 0;
    return v;
}

void synchronize(comm* c) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (!c) throw error(COSTA_ERR_ARG, "costa: null communicator");
    device_ctx& dc = ctx(c->device);
    HIP_CHECK(hipStreamSynchronize(dc.main));
    HIP_CHECK(hipStreamSynchronize(dc.aux));
    HIP_CHECK(hipStreamSynchronize(dc.xch));
    dc.resolve();
}

namespace {
// The exchange: one RCCL group of ncclSend / ncclRecv, one pair per peer, at the reference's
// displacements (communication_data.cpp:152-154).  Each peer's package moves as pieces of at
// most max_message_bytes(): RCCL was measured to lose the second half of a single >1 GiB self
// send/recv (tools/loopback_probe.py); pieces to one peer match in issue order on both sides.
// Round `round` of `rounds` (exchange_rounds(); rounds = 1: everything at once).
void issue_exchange(comm* c, const plan& p, char* sb, char* rb, hipStream_t s, int round = 0,
                    int rounds = 1) {
    const size_t E = pkg_unit_size(p.pkg_dtype);
    const size_t piece = max_message_bytes();
    NCCL_CHECK(ncclGroupStart());
    for (int q = 0; q < c->size; ++q) {
        int64_t slo, shi, rlo, rhi;
        round_range(p.send_counts[size_t(q)], E, rounds, round, slo, shi);
        round_range(p.recv_counts[size_t(q)], E, rounds, round, rlo, rhi);
        const size_t sbytes = size_t(shi - slo) * E, rbytes = size_t(rhi - rlo) * E;
        char* sp = sb + size_t(p.send_displs[size_t(q)] + slo) * E;
        char* rp = rb + size_t(p.recv_displs[size_t(q)] + rlo) * E;
        for (size_t o = 0; o < sbytes; o += piece)
            NCCL_CHECK(ncclSend(sp + o, std::min(piece, sbytes - o), ncclUint8, q, c->nccl, s));
        for (size_t o = 0; o < rbytes; o += piece)
            NCCL_CHECK(ncclRecv(rp + o, std::min(piece, rbytes - o), ncclUint8, q, c->nccl, s));
    }
    NCCL_CHECK(ncclGroupEnd());
}

// The scale scheme of a call over a scaled plan and its arguments (of the call, not of the plan).  The
// kernel family the plan's scaled LOCAL / UNPACK lists run on (launch_phase) and the item counter they
// add to (count_phase) follow from the tag: a new scheme is a tag with its payload here and a case in
// each of those two.
enum class scale_scheme { none, vectors, mx, block, mx_dual };
struct scaled_args {
    scale_scheme scheme = scale_scheme::none;
    struct {  // vectors (costa_hip_transform_scaled, _amax): scaled_kernel reads the scales, updates the amax outputs
        const void *row_scale = nullptr, *col_scale = nullptr;
        void *row_amax = nullptr, *col_amax = nullptr;
    } vec;
    struct {  // mx (costa_hip_transform_mx): mx_kernel, its tensors in target coordinates
        mx_side a_scales, c_scales;
        mx_side ct_scales;  // costa_hip_transform_mx_dual: output 2's tensor, in Ct's coordinates; the
                            // plan's dual lists run on mx_dual_kernel
        bool ceil = false;
        bool sr = false;  // costa_hip_transform_mx_sr: the SR instances, with the keys of the call's seed
        mx_sr keys;
    } mx;
    struct {  // block (costa_hip_transform_block_scaled): block_kernel
        block_side a_scales, c_scales;
        bool pow2 = false;
    } blk;
    bool amax() const { return vec.row_amax || vec.col_amax; }
    // block_kernel's quantising form: over the 128 x 128 regions instead of the plan's sub-tiles
    bool quantises() const { return scheme == scale_scheme::block && blk.c_scales.data; }
};

// the matrix a layout describes
void layout_extent(const elayout& L, int64_t& rows, int64_t& cols) {
    rows = L.rows_split.empty() ? 0 : int64_t(L.rows_split.back()) - L.rows_split.front();
    cols = L.cols_split.empty() ? 0 : int64_t(L.cols_split.back()) - L.cols_split.front();
}

// The argument checks that costa_hip_transform_mx and costa_hip_transform_block_scaled (`who`) share,
// behind the pair's own: mask, aliasing, a descriptor on exactly the wanted sides, the rounding mode,
// beta, and each descriptor against its matrix (`check`: check_mx_scales / check_block_scales).
template <typename Scales>
void check_scale_job(const std::string& who, const job& j, bool want_a, bool want_c, const Scales& sa,
                     const Scales& sc, bool rounding_ok, const char* rounding_modes,
                     void (*check)(const Scales&, int64_t, int64_t, const std::string&)) {
    const std::string pair = std::string(dtype_name(j.A->dtype)) + " -> " + dtype_name(j.C->dtype);
    if (j.uplo != 'A') throw error(COSTA_ERR_ARG, who + "no triangular mask");
    if (j.A == j.C) throw error(COSTA_ERR_ARG, who + "in-place calls are not supported");
    if (want_a && !sa.data) throw error(COSTA_ERR_ARG, who + "a_scales is required for " + pair);
    if (!want_a && sa.data) throw error(COSTA_ERR_ARG, who + "a_scales given for a FLOAT source (" + pair + ")");
    if (want_c && !sc.data) throw error(COSTA_ERR_ARG, who + "c_scales is required for " + pair);
    if (!want_c && sc.data)
        throw error(COSTA_ERR_ARG, who + "c_scales given for a FLOAT destination (" + pair + ")");
    if (!rounding_ok) throw error(COSTA_ERR_ARG, who + "rounding must be " + rounding_modes);
    if (want_c) {
        float beta;
        std::memcpy(&beta, j.s.beta.data(), sizeof beta);
        if (!(beta == 0.0f)) throw error(COSTA_ERR_ARG, who + "beta must be 0 with c_scales");
    }
    int64_t r, k;
    if (want_a) {
        layout_extent(*j.A, r, k);
        check(sa, r, k, who + "a_scales");
    }
    if (want_c) {
        layout_extent(*j.C, r, k);
        check(sc, r, k, who + "c_scales");
    }
}

// The argument checks of costa_hip_transform_mx that need no plan and no device: the pair, which
// descriptors it wants, beta, the rounding mode, strides and aliasing.
void check_mx_job(const job& j) {
    const costa_dtype_t a = j.A->dtype, c = j.C->dtype;
    if (!mx_pair(a, c))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_transform_mx: no MX transform for ") + dtype_name(a) +
                                       " -> " + dtype_name(c) +
                                       (dtype_is_fp6(a) || dtype_is_fp6(c)
                                            ? " (FLOAT -> FP6, FP6 -> FLOAT, FP6 -> the same FP6)"
                                        : dtype_is_fp4(a) || dtype_is_fp4(c)
                                            ? " (FLOAT -> FP4_E2M1, FP4_E2M1 -> FLOAT, FP4_E2M1 -> FP4_E2M1)"
                                            : " (FLOAT -> FP8, FP8 -> FLOAT, FP8 -> the same FP8)"));
    check_scale_job("costa_hip_transform_mx: ", j, dtype_is_fp8(a) || dtype_is_packed(a),
                    dtype_is_fp8(c) || dtype_is_packed(c), j.a_scales, j.c_scales,
                    j.mx_rounding == COSTA_MX_FLOOR || j.mx_rounding == COSTA_MX_CEIL,
                    "COSTA_MX_FLOOR or COSTA_MX_CEIL", check_mx_scales);
    if (j.mx_sr && c == COSTA_FLOAT)
        throw error(COSTA_ERR_ARG, std::string("costa_hip_transform_mx_sr: stochastic rounding needs a quantising "
                                               "pair (c_scales), not ") + dtype_name(a) + " -> " + dtype_name(c));
}

// ... and of costa_hip_transform_block_scaled
void check_block_job(const job& j) {
    const std::string who = "costa_hip_transform_block_scaled: ";
    const costa_dtype_t a = j.A->dtype, c = j.C->dtype;
    if (!block_pair(a, c))
        throw error(COSTA_ERR_ARG, who + "no block-scaled transform for " + dtype_name(a) + " -> " + dtype_name(c) +
                                       " (FLOAT -> FP8, FP8 -> FLOAT, FP8 -> the same FP8)");
    check_scale_job(who, j, dtype_is_fp8(a), dtype_is_fp8(c), j.a_blocks, j.c_blocks,
                    j.blk_rounding == COSTA_BLOCK_EXACT || j.blk_rounding == COSTA_BLOCK_POW2,
                    "COSTA_BLOCK_EXACT or COSTA_BLOCK_POW2", check_block_scales);
}

// a descriptor as the kernel sees it: in target coordinates (`swap`: the tensor is indexed by A's
// matrix of a transposing job, whose rows are target columns)
mx_side mx_side_of(const costa_mx_scales_t& s, bool swap) {
    mx_side o;
    o.data = s.data;
    o.block_stride = s.block_stride;
    o.line_stride = s.line_stride;
    o.rows = (s.axis == COSTA_MX_ROWS) != swap;
    return o;
}

block_side block_side_of(const costa_block_scales_t& s, bool swap) {
    block_side o;
    o.data = s.data;
    if (!s.data) return o;
    o.row_stride = swap ? s.col_stride : s.row_stride;
    o.col_stride = swap ? s.row_stride : s.col_stride;
    o.row_shift = (swap ? s.block_cols : s.block_rows) == 128 ? 7 : 0;
    o.col_shift = (swap ? s.block_rows : s.block_cols) == 128 ? 7 : 0;
    return o;
}

// the scale tensors of an MX or block-scaled entry point (`who`) are in device memory
void scale_tensors_on_device(const std::string& who, const void* a_scales, const void* c_scales) {
    for (const void* v : {a_scales, c_scales})
        if (v && !is_device_ptr(v)) throw error(COSTA_ERR_ARG, who + ": the scale tensors must be device-resident");
}

// The tile-boundary rule of a plan's scaled ops for one kind of c_scales, `check` throwing where it
// fails; `rule` keeps the outcome with the plan: 0 not checked yet, 1 holds, -1 fails (a failing plan
// is checked again: the error carries the op).
template <typename Check>
void check_rule_once(int& rule, const cached_plan& cp, const elayout& C, Check check) {
    if (rule > 0) return;
    int64_t m, n;
    layout_extent(C, m, n);
    rule = -1;
    check(cp.p->local_scaled, m, n);
    check(cp.p->unpack_scaled, m, n);
    rule = 1;
}

// The checks of those two calls that need the plan and the device: residency of the tensors and the
// tile-boundary rule (kept per plan and axis / block shape); -> the call's arguments
scaled_args mx_args(const job& j, cached_plan& cp) {
    scale_tensors_on_device("costa_hip_transform_mx", j.a_scales.data, j.c_scales.data);
    if (j.c_scales.data)
        check_rule_once(cp.mx_rule[j.c_scales.axis == COSTA_MX_ROWS ? 0 : 1], cp, *j.C,
                        [&](const std::vector<costa_scaled_op_t>& ops, int64_t m, int64_t n) {
                            check_mx_ops(ops, j.c_scales.axis, m, n);
                        });
    scaled_args sv;
    sv.scheme = scale_scheme::mx;
    sv.mx.a_scales = mx_side_of(j.a_scales, std::toupper(static_cast<unsigned char>(j.trans)) != 'N');
    sv.mx.c_scales = mx_side_of(j.c_scales, false);
    sv.mx.ceil = j.mx_rounding == COSTA_MX_CEIL;
    sv.mx.sr = j.mx_sr;
    if (j.mx_sr) sv.mx.keys = mx_sr_keys(j.mx_seed);
    return sv;
}

// The argument checks of costa_hip_transform_mx_dual that need no plan and no device (costa_hip.h,
// "Dual-output MX quantise", "Other checks")
void check_dual_job(const job& j) {
    const std::string who = "costa_hip_transform_mx_dual: ";
    const costa_dtype_t a = j.A->dtype, c = j.C->dtype, ct = j.Ct->dtype;
    if (a != COSTA_FLOAT)
        throw error(COSTA_ERR_ARG, who + "A must be COSTA_FLOAT, not " + dtype_name(a) +
                                       " (no dual MX transform from a quantised or half source)");
    if (c != ct || c == COSTA_FLOAT || !mx_pair(COSTA_FLOAT, c))
        throw error(COSTA_ERR_ARG, who + "no dual MX transform for FLOAT -> " + dtype_name(c) + " / " + dtype_name(ct) +
                                       " (C and Ct of one type: FP8_E4M3, FP8_E5M2, FP4_E2M1, FP6_E2M3 or FP6_E3M2)");
    if (j.uplo != 'A') throw error(COSTA_ERR_ARG, who + "no triangular mask");
    if (j.A == j.C) throw error(COSTA_ERR_ARG, who + "in-place calls are not supported");
    if (j.Ct == j.A || j.Ct == j.C)
        throw error(COSTA_ERR_ARG, who + "Ct must be a layout of its own, not the same object as " +
                                       (j.Ct == j.A ? "A" : "C"));
    int64_t m, n, r, k;
    layout_extent(*j.C, m, n);
    layout_extent(*j.Ct, r, k);
    if (r != n || k != m)
        throw error(COSTA_ERR_ARG, who + "dual layouts: Ct describes a " + std::to_string(r) + " x " + std::to_string(k) +
                                       " matrix, the transpose of C's " + std::to_string(m) + " x " + std::to_string(n) +
                                       " is " + std::to_string(n) + " x " + std::to_string(m));
    if (!j.c_scales.data) throw error(COSTA_ERR_ARG, who + "c_scales is required");
    if (!j.ct_scales.data) throw error(COSTA_ERR_ARG, who + "ct_scales is required");
    if (j.mx_rounding != COSTA_MX_FLOOR && j.mx_rounding != COSTA_MX_CEIL)
        throw error(COSTA_ERR_ARG, who + "rounding must be COSTA_MX_FLOOR or COSTA_MX_CEIL");
    check_mx_scales(j.c_scales, m, n, who + "c_scales");
    check_mx_scales(j.ct_scales, n, m, who + "ct_scales");
}

// ... and those that need the plan and the device; -> the call's arguments
scaled_args dual_args(const job& j, cached_plan& cp) {
    scale_tensors_on_device("costa_hip_transform_mx_dual", j.c_scales.data, j.ct_scales.data);
    int& rule = cp.dual_rule[j.c_scales.axis == COSTA_MX_ROWS ? 0 : 1][j.ct_scales.axis == COSTA_MX_ROWS ? 0 : 1];
    if (rule <= 0) {  // (a failing plan is checked again: the error carries the op)
        int64_t m, n;
        layout_extent(*j.C, m, n);
        rule = -1;
        check_dual_ops(cp.p->dtype, cp.local_dual, j.c_scales.axis, j.ct_scales.axis, m, n);
        check_dual_ops(cp.p->dtype, cp.unpack_dual, j.c_scales.axis, j.ct_scales.axis, m, n);
        rule = 1;
    }
    scaled_args sv;
    sv.scheme = scale_scheme::mx_dual;
    sv.mx.c_scales = mx_side_of(j.c_scales, false);
    sv.mx.ct_scales = mx_side_of(j.ct_scales, false);
    sv.mx.ceil = j.mx_rounding == COSTA_MX_CEIL;
    sv.mx.sr = j.mx_sr;
    if (j.mx_sr) sv.mx.keys = mx_sr_keys(j.mx_seed);
    return sv;
}

scaled_args block_args(const job& j, cached_plan& cp) {
    scale_tensors_on_device("costa_hip_transform_block_scaled", j.a_blocks.data, j.c_blocks.data);
    if (j.c_blocks.data)
        check_rule_once(cp.blk_rule[j.c_blocks.block_rows == 1 ? 0 : j.c_blocks.block_cols == 1 ? 1 : 2], cp, *j.C,
                        [&](const std::vector<costa_scaled_op_t>& ops, int64_t m, int64_t n) {
                            check_block_ops(ops, j.c_blocks.block_rows, j.c_blocks.block_cols, m, n);
                        });
    scaled_args sv;
    sv.scheme = scale_scheme::block;
    sv.blk.a_scales = block_side_of(j.a_blocks, std::toupper(static_cast<unsigned char>(j.trans)) != 'N');
    sv.blk.c_scales = block_side_of(j.c_blocks, false);
    sv.blk.pow2 = j.blk_rounding == COSTA_BLOCK_POW2;
    return sv;
}

// One phase of a transform on stream s: LOCAL, one round's PACK into the send package (dst_base) or
// one round's UNPACK from the receive package (src_base).  The launches keep their order -- converting
// list, tile_kernel list, edge tiles, scaled list -- and each waits for `after` (a round's exchange;
// null: nothing to wait for) and has its own timing bracket.  transform() calls it for an RCCL
// communicator (on the context's three streams, around issue_exchange) and for the selected part of
// an emulated one (on main, against the caller's package).
void launch_phase(const cached_plan& cp, const phase_lists& ph, list_kind kind, const char* src_base,
                  char* dst_base, const scaled_args& sv, phase_timer& tm, hipStream_t s,
                  hipEvent_t after = nullptr) {
    const dtype_pair t = phase_dtypes(*cp.p, kind);
    const int id = kind == list_local ? PH_LOCAL : kind == list_pack ? PH_PACK : PH_UNPACK;
    const void* scal = cp.d_scal.p;
    auto launch = [&](int phase, auto&& run) {
        if (after) HIP_CHECK(hipStreamWaitEvent(s, after, 0));
        tm.start(phase, s);
        run();
        tm.stop();
    };
    if (ph.convert.n_items)
        launch(id, [&] {
            launch_convert(t.src, t.dst, ph.tiles.list<costa_tile_op_t>(), ph.tiles.items(), ph.convert, src_base,
                           dst_base, scal, s);
        });
    if (ph.split.n_items())
        launch(id, [&] {
            launch_tiles(t.dst,
                         make_launch(ph.split, ph.tiles.ops.p, ph.tiles.work.p, src_base, dst_base, scal,
                                     ph.transposes, ph.reads_c),
                         s);
        });
    if (ph.tri_items.n_items)  // the edge tiles of a triangular plan, behind its ordinary list
        launch(kind == list_local ? PH_TRI_LOCAL : PH_TRI_UNPACK, [&] {
            launch_tri(t.dst, ph.tri.list<costa_tri_op_t>(), ph.tri.items(), ph.tri_items, src_base, dst_base, scal, s);
        });
    if (ph.scaled_items.n_items)  // the list of a scaled plan, on the kernels of the call's scheme
        launch(id, [&] {
            const costa_scaled_op_t* ops = ph.scaled.list<costa_scaled_op_t>();
            switch (sv.scheme) {
            case scale_scheme::block:
                launch_block(t.src, t.dst, ops,
                             sv.quantises() ? static_cast<const uint64_t*>(ph.block_work.p) : ph.scaled.items(),
                             sv.quantises() ? ph.block_items : ph.scaled_items, src_base, dst_base, scal,
                             sv.blk.a_scales, sv.blk.c_scales, sv.blk.pow2, s);
                break;
            case scale_scheme::mx:
                launch_mx(t.src, t.dst, ops, ph.scaled.items(), ph.scaled_items, src_base, dst_base, scal,
                          sv.mx.a_scales, sv.mx.c_scales, sv.mx.ceil, s, sv.mx.sr ? &sv.mx.keys : nullptr);
                break;
            default:
                launch_scaled(t.src, t.dst, ops, ph.scaled.items(), ph.scaled_items, src_base, dst_base, scal,
                              sv.vec.row_scale, sv.vec.col_scale, sv.vec.row_amax, sv.vec.col_amax, s);
            }
        });
    if (ph.dual_items.n_items)  // the list of a dual-output MX plan: both outputs in one launch
        launch(id, [&] {
            if (sv.scheme != scale_scheme::mx_dual)
                throw error(COSTA_ERR_INTERNAL, "costa: a dual-output plan outside costa_hip_transform_mx_dual");
            launch_mx_dual(t.dst, ph.dual.list<costa_dual_op_t>(), ph.dual.items(), ph.dual_items, src_base, dst_base,
                           nullptr, scal, sv.mx.c_scales, sv.mx.ct_scales, sv.mx.ceil, s,
                           sv.mx.sr ? &sv.mx.keys : nullptr);
        });
}

// the statistics of those launches
void count_items(const plan& p, const work_split& w) {
    g_stats.tile_items += w.n_large + w.n_medium;
    g_stats.skew_items += w.n_skew;
    g_stats.cblock_items += w.n_cblock;
    g_stats.tiny_items += w.n_tiny;
    if (!dtype_is_complex(p.dtype) && pieces_in_group_launch(w.n_cblock, w.n_tiny))
        g_stats.fused_pieces += w.n_tiny;
}

// (a phase counts as one launch where any of its lists is non-empty; LOCAL's bytes with it, the
// packages' bytes with the whole exchange)
void count_phase(const plan& p, const phase_lists& ph, list_kind kind, const scaled_args& sv) {
    if (!ph.empty()) {
        (kind == list_local ? g_stats.local_launches : kind == list_pack ? g_stats.pack_launches
                                                                         : g_stats.unpack_launches)++;
        if (kind == list_local) g_stats.local_bytes += p.local_bytes;
    }
    count_items(p, ph.split);
    g_stats.convert_items += ph.convert.n_items;
    g_stats.tri_items += ph.tri_items.n_items;
    const int64_t n = ph.scaled_items.n_items;
    switch (sv.scheme) {
    case scale_scheme::block: g_blk_items += sv.quantises() ? ph.block_items.n_items : n; break;
    case scale_scheme::mx: g_mx_items += n; break;
    default: g_scaled_items += n;
    }
    if (sv.amax()) g_amax_items += n;
    g_mx_dual_items += ph.dual_items.n_items;
}


// whether the device allocation around `buffer` has `bytes` bytes from it on (true where the
// runtime cannot tell)
bool buffer_holds(const void* buffer, size_t bytes) {
    hipDeviceptr_t base = nullptr;
    size_t sz = 0;
    if (hipMemGetAddressRange(&base, &sz, const_cast<void*>(buffer)) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    const size_t off = size_t(static_cast<const char*>(buffer) - static_cast<const char*>(base));
    return off <= sz && sz - off >= bytes;
}

// The selected part of an emulated communicator (comm_emulate), on main: the same lists and
// launches as below, the exchange being the caller's copies between the ranks' packages.  The
// plan's pack_bytes / unpack_bytes are counted with the last round, `transforms` with LOCAL.
void run_emulated_part(const comm* c, device_ctx& dc, const cached_plan& cp, const scaled_args& sv) {
    const plan& p = *cp.p;
    const size_t E = pkg_unit_size(p.pkg_dtype);
    phase_timer tm(dc, g_profiling);
    const int R = int(cp.rounds.size());
    const int r0 = c->round < 0 ? 0 : c->round, r1 = c->round < 0 ? R : c->round + 1;
    if (c->part == COSTA_EMULATE_LOCAL) {
        launch_phase(cp, cp.local, list_local, nullptr, nullptr, sv, tm, dc.main);
        count_phase(p, cp.local, list_local, sv);
        g_stats.transforms++;
    } else if (c->part == COSTA_EMULATE_PACK) {
        if (!buffer_holds(c->buffer, size_t(p.send_elems) * E))
            throw error(COSTA_ERR_ARG, "costa: the emulated send package is smaller than the plan's");
        for (int r = r0; r < r1; ++r) {
            const phase_lists& pack = cp.rounds[size_t(r)]->pack;
            launch_phase(cp, pack, list_pack, nullptr, static_cast<char*>(c->buffer), sv, tm, dc.main);
            count_phase(p, pack, list_pack, sv);
        }
        if (r1 == R) g_stats.pack_bytes += p.pack_bytes;
    } else {
        if (!buffer_holds(c->buffer, size_t(p.recv_elems) * E))
            throw error(COSTA_ERR_ARG, "costa: the emulated receive package is smaller than the plan's");
        for (int r = r0; r < r1; ++r) {
            const phase_lists& unpack = cp.rounds[size_t(r)]->unpack;
            launch_phase(cp, unpack, list_unpack, static_cast<const char*>(c->buffer), nullptr, sv, tm, dc.main);
            count_phase(p, unpack, list_unpack, sv);
        }
        if (r1 == R) g_stats.unpack_bytes += p.unpack_bytes;
    }
    HIP_CHECK(hipStreamSynchronize(dc.main));
    dc.resolve();
}

}  // namespace

void transform(const std::vector<job>& jobs, comm* c, void* user_stream, bool async) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (!c) throw error(COSTA_ERR_ARG, "costa: null communicator");
    device_ctx& dc = ctx(c->device);
    if (c->emulated) {  // test mode: one part of the transform against the caller's package
        if (c->part == 0)
            throw error(COSTA_ERR_ARG, "costa: an emulated communicator with no part selected "
                                       "(costa_hip_comm_emulate)");
        if (async)
            throw error(COSTA_ERR_ARG, "costa: an emulated communicator runs blocking transforms only "
                                       "(no _async form)");
        for (const job& j : jobs)
            if (!layout_on_device(*j.A) || !layout_on_device(*j.C))
                throw error(COSTA_ERR_ARG, "costa: an emulated communicator needs device-resident layouts");
    }
    const bool dual = jobs.size() == 1 && jobs[0].Ct;
    const bool mx = jobs.size() == 1 && jobs[0].mx && !dual;
    if (!mx && !dual && any_packed(jobs)) {  // (before any residency or staging question)
        costa_dtype_t a, b;
        check_jobs(jobs, c->size, a, b);
    }
    if (mx) check_mx_job(jobs[0]);  // pair, descriptors, beta, strides: before the plan
    if (dual) {
        check_dual_job(jobs[0]);
        for (const elayout* L : {jobs[0].A, jobs[0].C, jobs[0].Ct})
            if (!layout_on_device(*L))
                throw error(COSTA_ERR_ARG, "costa_hip_transform_mx_dual: A, C and Ct must be device-resident layouts");
    }
    const bool blk = !jobs.empty() && jobs[0].blk;
    if (blk) check_block_job(jobs[0]);
    cached_plan& cp = *get_plan(jobs, c, dc);
    const plan& p = *cp.p;
    const size_t E = pkg_unit_size(p.pkg_dtype);  // of the send / receive packages
    scaled_args sv;
    if (blk) {
        sv = block_args(jobs[0], cp);
    } else if (dual) {
        sv = dual_args(jobs[0], cp);
    } else if (mx) {
        sv = mx_args(jobs[0], cp);
    } else if (p.scaled) {
        // the vectors of a scaled transform: arguments of this call, read by its LOCAL / UNPACK kernels
        // ... and its amax outputs, updated by the same kernels (costa_hip_transform_amax)
        sv.scheme = scale_scheme::vectors;
        sv.vec = {jobs[0].row_scale, jobs[0].col_scale, jobs[0].row_amax, jobs[0].col_amax};
        if (!sv.vec.row_scale && !sv.vec.col_scale && !sv.amax())
            throw error(COSTA_ERR_ARG, "costa: a scaled transform without scale vectors (use costa_hip_transform)");
        for (const void* v : {sv.vec.row_scale, sv.vec.col_scale})
            if (v && !is_device_ptr(v))
                throw error(COSTA_ERR_ARG, "costa: the scale vectors of a scaled transform must be "
                                           "device-resident");
        for (const void* v : {static_cast<const void*>(sv.vec.row_amax), static_cast<const void*>(sv.vec.col_amax)})
            if (v && !is_device_ptr(v))
                throw error(COSTA_ERR_ARG, "costa: the amax vectors of a scaled transform must be "
                                           "device-resident");
    }
    if (async && (cp.staged || cp.pipe))
        throw error(COSTA_ERR_ARG,
                    "costa: asynchronous transforms need device-resident layouts (host data is "
                    "staged synchronously)");
    hipStream_t user = static_cast<hipStream_t>(user_stream);
    // everything runs on the context's streams, in call order (they own the workspaces);
    // a caller stream is joined at entry and made to wait for the result at exit
    if (user) {
        HIP_CHECK(hipEventRecord(dc.ev_user, user));
        HIP_CHECK(hipStreamWaitEvent(dc.main, dc.ev_user, 0));
    }
    upload_scalars(cp, jobs, dc.main);
    if (cp.pipe) {  // host-resident: pipelined gather -> H2D -> [exchange] -> kernels -> D2H
        const bool xchg = c->nccl != nullptr && (p.send_elems > 0 || p.recv_elems > 0);
        char *sb = nullptr, *rb = nullptr;
        std::function<void(void*, int)> fn;
        if (xchg) {
            dc.send.reserve(size_t(p.send_elems) * E + 256);
            dc.recv.reserve(size_t(p.recv_elems) * E + 256);
            sb = static_cast<char*>(dc.send.p);
            rb = static_cast<char*>(dc.recv.p);
            const int R = exchange_rounds();
            fn = [&, R](void* s, int r) {
                issue_exchange(c, p, sb, rb, static_cast<hipStream_t>(s), r, R);
            };
        }
        // tile kernels on the aux stream, behind the scalars uploaded on main; the exchange on main
        HIP_CHECK(hipEventRecord(dc.ev_ready, dc.main));
        HIP_CHECK(hipStreamWaitEvent(dc.aux, dc.ev_ready, 0));
        run_host_pipeline(*cp.pipe, c->device, dc.aux, dc.main, sb, rb, fn, cp.d_scal.p);
        g_stats.transforms++;
        return;
    }
    if (c->emulated) return run_emulated_part(c, dc, cp, sv);
    phase_timer tm(dc, g_profiling);

    // H2D of host-resident data
    if (cp.staged) {
        tm.start(PH_H2D, dc.main);
        for (const auto& r : cp.h2d_ranges)
            HIP_CHECK(hipMemcpyAsync(static_cast<char*>(cp.stage.p) + r.dev_off,
                                     reinterpret_cast<void*>(r.lo), r.hi - r.lo,
                                     hipMemcpyHostToDevice, dc.main));
        tm.stop();
    }

    const bool exchange = c->nccl != nullptr && (p.send_elems > 0 || p.recv_elems > 0);
    // LOCAL on the aux stream when there is an exchange to overlap, else on main
    hipStream_t ls = exchange ? dc.aux : dc.main;
    if (exchange) {
        HIP_CHECK(hipEventRecord(dc.ev_ready, dc.main));
        HIP_CHECK(hipStreamWaitEvent(dc.aux, dc.ev_ready, 0));
    }
    launch_phase(cp, cp.local, list_local, nullptr, nullptr, sv, tm, ls);

    if (exchange) {
        dc.send.reserve(size_t(p.send_elems) * E + 256);
        dc.recv.reserve(size_t(p.recv_elems) * E + 256);
        char* sb = static_cast<char*>(dc.send.p);
        char* rb = static_cast<char*>(dc.recv.p);
        // main: pack round r -> the exchange stream moves round r -> aux (after LOCAL): unpack
        // round r; so packing r+1, moving r and unpacking r-1 overlap
        const int R = int(cp.rounds.size());
        dc.round_events(size_t(R));
        for (int r = 0; r < R; ++r) {
            launch_phase(cp, cp.rounds[size_t(r)]->pack, list_pack, nullptr, sb, sv, tm, dc.main);
            HIP_CHECK(hipEventRecord(dc.ev_packed[size_t(r)], dc.main));
            HIP_CHECK(hipStreamWaitEvent(dc.xch, dc.ev_packed[size_t(r)], 0));
            tm.start(PH_EXCHANGE, dc.xch);
            issue_exchange(c, p, sb, rb, dc.xch, r, R);
            tm.stop();
            HIP_CHECK(hipEventRecord(dc.ev_moved[size_t(r)], dc.xch));
        }
        for (int r = 0; r < R; ++r)
            launch_phase(cp, cp.rounds[size_t(r)]->unpack, list_unpack, rb, nullptr, sv, tm, dc.aux,
                         dc.ev_moved[size_t(r)]);
        // the call ends on main once LOCAL, every unpack and every round of the exchange are done
        HIP_CHECK(hipEventRecord(dc.ev_local, dc.aux));
        HIP_CHECK(hipStreamWaitEvent(dc.main, dc.ev_local, 0));
        HIP_CHECK(hipStreamWaitEvent(dc.main, dc.ev_moved[size_t(R - 1)], 0));
    }

    // D2H of the target data
    if (cp.staged) {
        tm.start(PH_D2H, dc.main);
        for (const auto& r : cp.d2h_ranges)
            HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(r.lo),
                                     static_cast<char*>(cp.stage.p) + r.dev_off, r.hi - r.lo,
                                     hipMemcpyDeviceToHost, dc.main));
        tm.stop();
    }

    g_stats.transforms++;
    count_phase(p, cp.local, list_local, sv);
    if (exchange) {
        for (const auto& x : cp.rounds) {
            count_phase(p, x->pack, list_pack, sv);
            count_phase(p, x->unpack, list_unpack, sv);
        }
        g_stats.pack_bytes += p.pack_bytes;
        g_stats.unpack_bytes += p.unpack_bytes;
    }

    if (async) {
        if (user) {  // (no marker without a caller stream: each one widened the gap between calls)
            HIP_CHECK(hipEventRecord(dc.ev_done, dc.main));
            HIP_CHECK(hipStreamWaitEvent(user, dc.ev_done, 0));
        }
        return;
    }
    HIP_CHECK(hipStreamSynchronize(dc.main));
    dc.resolve();
}


// ---------------------------------------------------------------- direct tile calls
void execute_tiles(costa_dtype_t dtype, const costa_tile_op_t* ops, int64_t n,
                   const void* src_base, void* dst_base, const void* scalars, int n_slots,
                   int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (dtype_is_half(dtype) || dtype_is_fp8(dtype) || dtype_is_packed(dtype))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_execute_tiles: no same-type tile kernel for ") +
                                       dtype_name(dtype) + " (use costa_hip_execute_tiles_mixed)");
    device_ctx& dc = ctx(device);
    std::vector<costa_tile_op_t> v(ops, ops + n);
    for (const auto& op : v)
        if ((op.flags >> COSTA_SLOT_SHIFT) >= uint32_t(std::max(n_slots, 0)))
            throw error(COSTA_ERR_ARG, "costa_hip_execute_tiles: scalar slot out of range");
    std::vector<costa_tile_op_t> ord;
    std::vector<uint64_t> w;
    const work_split nl = build_work(dtype, v, ord, w);
    dbuf d_ops, d_work, d_scal;
    d_ops.upload(ord, dc.main);
    d_work.upload(w, dc.main);
    const size_t E = dtype_size(dtype);
    std::vector<unsigned char> sc(static_cast<const unsigned char*>(scalars),
                                  static_cast<const unsigned char*>(scalars) + size_t(n_slots) * 2 * E);
    d_scal.upload(sc, dc.main);
    launch_tiles(dtype,
                 make_launch(nl, d_ops.p, d_work.p, static_cast<const char*>(src_base),
                             static_cast<char*>(dst_base), d_scal.p, any_transpose(v),
                             any_axpby(v)),
                 dc.main);
    HIP_CHECK(hipStreamSynchronize(dc.main));
}

// ---------------------------------------------------------------- converting lists: the pair table
namespace {
const pair_family& family_of(costa_dtype_t src, costa_dtype_t dst) {  // every converting pair has one kernel family
    static const pair_family table[] = {half_family(), fp8_family(), wide_family()};
    for (const pair_family& f : table)
        if (f.has(src, dst)) return f;
    throw error(COSTA_ERR_ARG, std::string("costa: no converting kernel for ") + dtype_name(src) + " -> " +
                                   dtype_name(dst));
}
}  // namespace

void convert_subtile(costa_dtype_t src, costa_dtype_t dst, int* bf, int* bs) {
    family_of(src, dst).subtile(src, dst, bf, bs);
}

strip_list build_convert_work(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                              const std::vector<costa_tile_op_t>& ops, uint64_t src_base, uint64_t dst_base,
                              std::vector<costa_tile_op_t>& ordered, std::vector<uint64_t>& work) {
    int bf = 0, bs = 0;
    convert_subtile(src_dtype, dst_dtype, &bf, &bs);
    const uint64_t es = dtype_size(src_dtype), ed = dtype_size(dst_dtype);
    return build_strip_work("converting", ops, src_base, dst_base, bf, bs, es, ed,
                            strip_alignment(strip_family::pair, es, ed), ordered, work);
}

void launch_convert(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* d_ops,
                    const uint64_t* d_work, const strip_list& l, const char* src_base, char* dst_base,
                    const void* d_scalars, void* stream) {
    if (l.n_items <= 0) return;
    family_of(src_dtype, dst_dtype).launch(src_dtype, dst_dtype, d_ops, d_work, l, src_base, dst_base, d_scalars,
                                           stream);
}

namespace {
// One list of a strip kernel family, run to completion (costa_hip_execute_tiles_mixed, _tri, _scaled
// and _amax; `who` names the entry point): the ops are copied and their slots checked,
// build(ops, ordered, work) makes the work list, list, work and the n_slots (alpha, beta) pairs of
// `scalar_size` bytes each go to the device, launch(d_ops, d_work, list, d_scalars, stream) runs
// them.  Returns the sub-tiles run.
template <typename Op, typename Build, typename Launch>
int64_t run_strip_tiles(const std::string& who, const Op* ops, int64_t n, const void* scalars, int n_slots,
                        size_t scalar_size, int device, Build build, Launch launch) {
    device_ctx& dc = ctx(device);
    std::vector<Op> v(ops, ops + n);
    for (const Op& t : v)
        if ((tile_of(t).flags >> COSTA_SLOT_SHIFT) >= uint32_t(std::max(n_slots, 0)))
            throw error(COSTA_ERR_ARG, who + ": scalar slot out of range");
    std::vector<Op> ord;
    std::vector<uint64_t> w;
    const strip_list l = build(v, ord, w);
    if (!l.n_items) return 0;
    dbuf d_ops, d_work, d_scal;
    d_ops.upload(ord, dc.main);
    d_work.upload(w, dc.main);
    std::vector<unsigned char> sc(static_cast<const unsigned char*>(scalars),
                                  static_cast<const unsigned char*>(scalars) + size_t(n_slots) * 2 * scalar_size);
    d_scal.upload(sc, dc.main);
    launch(static_cast<const Op*>(d_ops.p), static_cast<const uint64_t*>(d_work.p), l, d_scal.p, dc.main);
    HIP_CHECK(hipStreamSynchronize(dc.main));
    return l.n_items;
}
}  // namespace

void execute_tiles_mixed(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_tile_op_t* ops,
                         int64_t n, const void* src_base, void* dst_base, const void* scalars,
                         int n_slots, int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (!convertible(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_execute_tiles_mixed: cannot convert ") +
                                       dtype_name(src_dtype) + " to " + dtype_name(dst_dtype) +
                                       " (FLOAT <-> DOUBLE, CFLOAT <-> CDOUBLE, and HALF or BFLOAT16 with "
                                       "itself or FLOAT only, and FP8_E4M3 or FP8_E5M2 with itself or FLOAT)");
    const uintptr_t sb = reinterpret_cast<uintptr_t>(src_base), db = reinterpret_cast<uintptr_t>(dst_base);
    g_stats.convert_items += run_strip_tiles(
        "costa_hip_execute_tiles_mixed", ops, n, scalars, n_slots,
        dtype_size(compute_dtype(src_dtype, dst_dtype)),  // (fp32 for half pairs)
        device, [&](const auto& v, auto& ord, auto& w) { return build_convert_work(src_dtype, dst_dtype, v, sb, db, ord, w); },
        [&](const costa_tile_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const void* d_scal, void* s) {
            launch_convert(src_dtype, dst_dtype, d_ops, d_work, l, static_cast<const char*>(src_base),
                           static_cast<char*>(dst_base), d_scal, s);
        });
}

void execute_tiles_tri(costa_dtype_t dtype, const costa_tri_op_t* ops, int64_t n, const void* src_base,
                       void* dst_base, const void* scalars, int n_slots, int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (dtype_is_half(dtype) || dtype_is_fp8(dtype) || dtype_is_packed(dtype))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_execute_tiles_tri: no edge-tile kernel for ") +
                                       dtype_name(dtype));
    const uintptr_t sb = reinterpret_cast<uintptr_t>(src_base), db = reinterpret_cast<uintptr_t>(dst_base);
    g_stats.tri_items += run_strip_tiles(
        "costa_hip_execute_tiles_tri", ops, n, scalars, n_slots, dtype_size(dtype), device,
        [&](const auto& v, auto& ord, auto& w) { return build_tri_work(dtype, v, sb, db, ord, w); },
        [&](const costa_tri_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const void* d_scal, void* s) {
            launch_tri(dtype, d_ops, d_work, l, static_cast<const char*>(src_base), static_cast<char*>(dst_base),
                       d_scal, s);
        });
}

namespace {
// costa_hip_execute_tiles_scaled (`who`, no amax vector) and costa_hip_execute_tiles_amax
void run_scaled_tiles(const std::string& who, costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                      const costa_scaled_op_t* ops, int64_t n, const void* src_base, void* dst_base,
                      const void* scalars, int n_slots, const void* row_scale, const void* col_scale,
                      void* row_amax, void* col_amax, int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    ctx(device);  // (is_device_ptr needs the device's context)
    for (const void* v : {row_scale, col_scale})
        if (v && !is_device_ptr(v))
            throw error(COSTA_ERR_ARG, who + ": the scale vectors must be device-resident");
    for (const void* v : {row_amax, col_amax})
        if (v && !is_device_ptr(v))
            throw error(COSTA_ERR_ARG, who + ": the amax vectors must be device-resident");
    const uintptr_t sb = reinterpret_cast<uintptr_t>(src_base), db = reinterpret_cast<uintptr_t>(dst_base);
    const int64_t items = run_strip_tiles(
        who, ops, n, scalars, n_slots, dtype_size(compute_dtype(src_dtype, dst_dtype)), device,
        [&](const auto& v, auto& ord, auto& w) { return build_scaled_work(src_dtype, dst_dtype, v, sb, db, ord, w, false); },
        [&](const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const void* d_scal, void* s) {
            launch_scaled(src_dtype, dst_dtype, d_ops, d_work, l, static_cast<const char*>(src_base),
                          static_cast<char*>(dst_base), d_scal, row_scale, col_scale, row_amax, col_amax, s);
        });
    g_scaled_items += items;
    if (row_amax || col_amax) g_amax_items += items;
}
}  // namespace

void execute_tiles_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                          int64_t n, const void* src_base, void* dst_base, const void* scalars,
                          int n_slots, const void* row_scale, const void* col_scale, int device) {
    if (!scaled_pair(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_execute_tiles_scaled: no scaled kernel for ") +
                                       dtype_name(src_dtype) + " -> " + dtype_name(dst_dtype));
    if (!row_scale && !col_scale)
        throw error(COSTA_ERR_ARG, "costa_hip_execute_tiles_scaled: no scale vector (use "
                                   "costa_hip_execute_tiles_mixed)");
    run_scaled_tiles("costa_hip_execute_tiles_scaled", src_dtype, dst_dtype, ops, n, src_base, dst_base,
                     scalars, n_slots, row_scale, col_scale, nullptr, nullptr, device);
}

void execute_tiles_amax(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                        int64_t n, const void* src_base, void* dst_base, const void* scalars, int n_slots,
                        const void* row_scale, const void* col_scale, void* row_amax, void* col_amax,
                        int device) {
    if (!scaled_pair(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_execute_tiles_amax: no scaled kernel for ") +
                                       dtype_name(src_dtype) + " -> " + dtype_name(dst_dtype));
    if (!row_amax && !col_amax)
        throw error(COSTA_ERR_ARG, "costa_hip_execute_tiles_amax: no amax vector (use "
                                   "costa_hip_execute_tiles_scaled)");
    run_scaled_tiles("costa_hip_execute_tiles_amax", src_dtype, dst_dtype, ops, n, src_base, dst_base,
                     scalars, n_slots, row_scale, col_scale, row_amax, col_amax, device);
}

// ---------------------------------------------------------------- costa_hip_layout_amax
std::vector<costa_scaled_op_t> layout_amax_ops(const elayout& L) {
    std::vector<costa_scaled_op_t> ops;
    if (L.rows_split.empty() || L.cols_split.empty()) return ops;
    const int r0 = L.rows_split.front(), c0 = L.cols_split.front();
    const bool col_major = L.ordering == 'C' || L.ordering == 'c';
    ops.reserve(L.blocks.size());
    for (const eblock& b : L.blocks) {
        if (!b.rows.non_empty() || !b.cols.non_empty()) continue;
        costa_scaled_op_t t{};
        t.op.src = reinterpret_cast<uintptr_t>(b.data);
        t.op.nf = col_major ? b.rows.length() : b.cols.length();
        t.op.ns = col_major ? b.cols.length() : b.rows.length();
        t.op.lds = b.ld;
        t.op.flags = col_major ? COSTA_SCALED_F_ROWS : 0u;
        t.row0 = b.rows.start - r0;
        t.col0 = b.cols.start - c0;
        if (t.op.lds < t.op.nf) throw error(COSTA_ERR_ARG, "costa: a block's leading dimension is below its extent");
        ops.push_back(t);
    }
    return ops;
}

void layout_amax(const elayout& L, void* row_amax, void* col_amax, comm* c, void* user_stream, bool async) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (!c) throw error(COSTA_ERR_ARG, "costa: null communicator");
    if (!amax_dtype(L.dtype))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_layout_amax: no amax of ") + dtype_name(L.dtype) +
                                       " (real floating-point element types only)");
    if (!row_amax && !col_amax)
        throw error(COSTA_ERR_ARG, "costa_hip_layout_amax: both amax vectors are NULL");
    device_ctx& dc = ctx(c->device);
    if (!layout_on_device(L))
        throw error(COSTA_ERR_ARG, "costa_hip_layout_amax: needs a device-resident layout");
    for (const void* v : {row_amax, col_amax})
        if (v && !is_device_ptr(v))
            throw error(COSTA_ERR_ARG, "costa_hip_layout_amax: the amax vectors must be device-resident");
    std::vector<costa_scaled_op_t> ord;
    std::vector<uint64_t> w;
    // (a source-only list: the destination side of build_scaled_work sees offset 0, ld 0)
    const strip_list l = build_scaled_work(L.dtype, L.dtype, layout_amax_ops(L), 0, 0, ord, w, false);
    hipStream_t user = static_cast<hipStream_t>(user_stream);
    if (user) {
        HIP_CHECK(hipEventRecord(dc.ev_user, user));
        HIP_CHECK(hipStreamWaitEvent(dc.main, dc.ev_user, 0));
    }
    if (l.n_items) {
        // the context's own lists: uploads and launches are ordered on main, so a list still read by
        // an earlier asynchronous call is overwritten only after that call's kernel
        dc.amax_ops.upload(ord, dc.main);
        dc.amax_work.upload(w, dc.main);
        launch_amax(L.dtype, static_cast<const costa_scaled_op_t*>(dc.amax_ops.p),
                    static_cast<const uint64_t*>(dc.amax_work.p), l.n_items, row_amax, col_amax, dc.main);
        g_amax_items += l.n_items;
    }
    if (async) {
        if (user) {
            HIP_CHECK(hipEventRecord(dc.ev_done, dc.main));
            HIP_CHECK(hipStreamWaitEvent(user, dc.ev_done, 0));
        }
        return;
    }
    HIP_CHECK(hipStreamSynchronize(dc.main));
}

int64_t amax_items(bool reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const int64_t v = g_amax_items;
    if (reset) g_amax_items = 0;
    return v;
}

int64_t scaled_items(bool reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const int64_t v = g_scaled_items;
    if (reset) g_scaled_items = 0;
    return v;
}

// ---------------------------------------------------------------- MX block-scaled transforms
void check_mx_scales(const costa_mx_scales_t& s, int64_t rows, int64_t cols, const std::string& what) {
    if (s.axis != COSTA_MX_ROWS && s.axis != COSTA_MX_COLS)
        throw error(COSTA_ERR_ARG, what + ": axis must be COSTA_MX_ROWS or COSTA_MX_COLS");
    if (s.block_stride <= 0 || s.line_stride <= 0)
        throw error(COSTA_ERR_ARG, what + ": the strides must be positive");
    const int64_t along = s.axis == COSTA_MX_ROWS ? rows : cols, lines = s.axis == COSTA_MX_ROWS ? cols : rows;
    const int64_t nb = (along + 31) / 32;
    // two positive strides address nb x lines distinct bytes exactly when the larger one steps over
    // the whole extent of the smaller one's index, or some pair (db, dl) with db*bs == dl*ls exists
    // inside the ranges: db < nb, dl < lines
    if (nb > 1 && lines > 1) {
        const int64_t g = std::gcd(s.block_stride, s.line_stride);
        // the smallest coincidence: db = ls / g, dl = bs / g
        if (s.line_stride / g < nb && s.block_stride / g < lines)
            throw error(COSTA_ERR_ARG, what + ": the strides make two (block, line) entries share a byte");
    }
}

void check_mx_ops(const std::vector<costa_scaled_op_t>& ops, int axis, int64_t m, int64_t n) {
    for (const costa_scaled_op_t& t : ops) {
        if (t.op.nf <= 0 || t.op.ns <= 0) continue;
        const bool frow = t.op.flags & COSTA_SCALED_F_ROWS;
        // the op's start and extent along the block axis, in C's coordinates
        const int64_t at = axis == COSTA_MX_ROWS ? t.row0 : t.col0;
        const int64_t len = (axis == COSTA_MX_ROWS) == frow ? t.op.nf : t.op.ns;
        const int64_t edge = axis == COSTA_MX_ROWS ? m : n;
        if (at % 32 != 0 || (len % 32 != 0 && at + len != edge) || at + len > edge)
            throw error(COSTA_ERR_ARG,
                        "costa: a tile boundary splits an MX block of C: a tile covers " +
                            std::string(axis == COSTA_MX_ROWS ? "rows " : "columns ") + std::to_string(at) + " .. " +
                            std::to_string(at + len) + " of " + std::to_string(edge) +
                            " (block sizes and split points of both layouts must be multiples of 32 along "
                            "c_scales.axis)");
    }
}

void check_packed_ops(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const std::vector<costa_scaled_op_t>& ops) {
    const int gs = std::max(1, packed_group(src_dtype)), gd = std::max(1, packed_group(dst_dtype));
    for (const costa_scaled_op_t& t : ops) {
        const costa_tile_op_t& op = t.op;
        if (op.nf <= 0 || op.ns <= 0) continue;
        // the source's stored-contiguous dimension is f; the destination's f (copy) or s (transpose)
        const bool tr = op.flags & COSTA_TILE_TRANSPOSE;
        const int64_t dn = tr ? op.ns : op.nf;
        const bool bad_src = op.nf % gs != 0 || op.lds % gs != 0;
        const bool bad_dst = dn % gd != 0 || op.ldd % gd != 0;
        if ((bad_src && dtype_is_fp6(src_dtype)) || (!bad_src && bad_dst && dtype_is_fp6(dst_dtype)))
            throw error(COSTA_ERR_ARG,
                        std::string("costa: FP6 quad: an op splits a 3-byte group of its ") +
                            dtype_name(bad_src ? src_dtype : dst_dtype) + (bad_src ? " source" : " destination") +
                            ": [0, " + std::to_string(bad_src ? int64_t(op.nf) : dn) +
                            ") elements along the stored-contiguous dimension with ld " +
                            std::to_string(bad_src ? op.lds : op.ldd) + " (both must be multiples of 4; target rows " +
                            std::to_string(t.row0) + " .., columns " + std::to_string(t.col0) + " ..)");
        if (bad_src || bad_dst)
            throw error(COSTA_ERR_ARG,
                        std::string("costa: FP4 pair: an op splits a byte of its FP4_E2M1 ") +
                            (bad_src ? "source" : "destination") + ": [0, " +
                            std::to_string(bad_src ? int64_t(op.nf) : dn) + ") elements along the stored-contiguous "
                            "dimension with ld " + std::to_string(bad_src ? op.lds : op.ldd) +
                            " (both must be even; target rows " + std::to_string(t.row0) + " .., columns " +
                            std::to_string(t.col0) + " ..)");
    }
}

namespace {
// the ops of costa_hip_execute_tiles_mx / _block_scaled (`who`) lie inside C's m x n matrix
void check_ops_inside(const std::string& who, const std::vector<costa_scaled_op_t>& ops, int64_t m, int64_t n) {
    for (const costa_scaled_op_t& t : ops) {
        if (t.op.nf <= 0 || t.op.ns <= 0) continue;
        if (t.row0 < 0 || t.col0 < 0) throw error(COSTA_ERR_ARG, who + ": negative target coordinate");
        const bool frow = t.op.flags & COSTA_SCALED_F_ROWS;
        if (t.row0 + int64_t(frow ? t.op.nf : t.op.ns) > m || t.col0 + int64_t(frow ? t.op.ns : t.op.nf) > n)
            throw error(COSTA_ERR_ARG, who + ": an op reaches past the m x n matrix");
    }
}
// ... and, under c_scales, none of them reads C
void check_no_axpby(const std::string& who, const std::vector<costa_scaled_op_t>& ops) {
    for (const costa_scaled_op_t& t : ops)
        if (((t.op.flags & COSTA_SCALE_MASK) >> COSTA_SCALE_SHIFT) == COSTA_SCALE_AXPBY)
            throw error(COSTA_ERR_ARG, who + ": beta must be 0 with c_scales (an op of kind AXPBY)");
}
}  // namespace

void execute_tiles_mx(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                      int64_t n_ops, const void* src_base, void* dst_base, const void* scalars, int n_slots,
                      const costa_mx_scales_t* a_scales, const costa_mx_scales_t* c_scales, int rounding,
                      int64_t m, int64_t n, int a_transposed, int device, const uint64_t* seed) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const std::string who = "costa_hip_execute_tiles_mx";
    if (!mx_pair(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, who + ": no MX kernel for " + dtype_name(src_dtype) + " -> " + dtype_name(dst_dtype));
    const costa_mx_scales_t none{};
    const costa_mx_scales_t& sa = a_scales && a_scales->data ? *a_scales : none;
    const costa_mx_scales_t& sc = c_scales && c_scales->data ? *c_scales : none;
    const bool p4 = dtype_is_fp4(src_dtype) || dtype_is_fp4(dst_dtype);
    const bool p6 = dtype_is_fp6(src_dtype) || dtype_is_fp6(dst_dtype);
    if ((sa.data != nullptr) != (src_dtype != COSTA_FLOAT) || (sc.data != nullptr) != (dst_dtype != COSTA_FLOAT))
        throw error(COSTA_ERR_ARG, who + ": a scale tensor is needed exactly on the " + (p6 ? "FP6" : p4 ? "FP4" : "FP8") +
                                       " sides of " + dtype_name(src_dtype) + " -> " + dtype_name(dst_dtype));
    if (rounding != COSTA_MX_FLOOR && rounding != COSTA_MX_CEIL)
        throw error(COSTA_ERR_ARG, who + ": rounding must be COSTA_MX_FLOOR or COSTA_MX_CEIL");
    if (m < 0 || n < 0) throw error(COSTA_ERR_ARG, who + ": negative matrix extent");
    if (sa.data) check_mx_scales(sa, a_transposed ? n : m, a_transposed ? m : n, who + ": a_scales");
    std::vector<costa_scaled_op_t> v(ops, ops + n_ops);
    check_ops_inside(who, v, m, n);
    if (sc.data) {
        check_mx_scales(sc, m, n, who + ": c_scales");
        check_no_axpby(who, v);
        check_mx_ops(v, sc.axis, m, n);
    }
    if (p4 || p6) check_packed_ops(src_dtype, dst_dtype, v);
    if (seed && dst_dtype == COSTA_FLOAT)
        throw error(COSTA_ERR_ARG, who + "_sr: stochastic rounding needs a quantising pair (c_scales), not " +
                                       dtype_name(src_dtype) + " -> " + dtype_name(dst_dtype));
    const mx_sr keys = seed ? mx_sr_keys(*seed) : mx_sr{};
    ctx(device);  // (is_device_ptr needs the device's context)
    scale_tensors_on_device(who, sa.data, sc.data);
    const mx_side da = mx_side_of(sa, a_transposed != 0), dc_ = mx_side_of(sc, false);
    const uintptr_t sb = reinterpret_cast<uintptr_t>(src_base), db = reinterpret_cast<uintptr_t>(dst_base);
    g_mx_items += run_strip_tiles(
        who, v.data(), n_ops, scalars, n_slots, sizeof(float), device,
        [&](const auto& l, auto& ord, auto& w) { return build_scaled_work(src_dtype, dst_dtype, l, sb, db, ord, w, false); },
        [&](const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const void* d_scal, void* s) {
            launch_mx(src_dtype, dst_dtype, d_ops, d_work, l, static_cast<const char*>(src_base),
                      static_cast<char*>(dst_base), d_scal, da, dc_, rounding == COSTA_MX_CEIL, s,
                      seed ? &keys : nullptr);
        });
}

int64_t mx_items(bool reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const int64_t v = g_mx_items;
    if (reset) g_mx_items = 0;
    return v;
}

// ---------------------------------------------------------------- dual-output MX quantise
costa_scaled_op_t dual_twin_op(const costa_dual_op_t& t) {
    costa_scaled_op_t o = t.s;
    o.op.dst = t.dst2;
    o.op.ldd = t.ldd2;
    o.op.flags = ((t.s.op.flags & ~uint32_t(COSTA_TILE_TRANSPOSE | COSTA_TILE_VEC_DST)) ^ COSTA_SCALED_F_ROWS) |
                 (t.flags2 & (COSTA_TILE_TRANSPOSE | COSTA_TILE_VEC_DST));
    o.row0 = t.s.col0;
    o.col0 = t.s.row0;
    return o;
}

std::vector<costa_dual_op_t> dual_twins(const std::vector<costa_scaled_op_t>& ops, const elayout& Ct, int rank) {
    std::vector<costa_dual_op_t> out;
    out.reserve(ops.size());
    if (ops.empty()) return out;
    const esize E = elem_size(Ct.dtype);
    const int g = std::max(1, packed_group(Ct.dtype));
    const bool ct_cm = Ct.ordering == 'C' || Ct.ordering == 'c';
    const int nbc = Ct.nbc();
    // Ct's local blocks by the grid cell of their first element
    std::unordered_map<int64_t, std::vector<const eblock*>> by_cell;
    auto cell_of = [](const std::vector<int>& split, int at) {
        return int(std::upper_bound(split.begin(), split.end(), at) - split.begin()) - 1;
    };
    for (const eblock& b : Ct.blocks) {
        if (!b.rows.non_empty() || !b.cols.non_empty()) continue;
        by_cell[int64_t(cell_of(Ct.rows_split, b.rows.start)) * nbc + cell_of(Ct.cols_split, b.cols.start)].push_back(&b);
    }
    const int rb = Ct.rows_split.empty() ? 0 : Ct.rows_split.front(), cb = Ct.cols_split.empty() ? 0 : Ct.cols_split.front();
    for (const costa_scaled_op_t& t : ops) {
        costa_dual_op_t d{};
        d.s = t;
        if (t.op.nf <= 0 || t.op.ns <= 0) {
            out.push_back(d);
            continue;
        }
        const bool frow = t.op.flags & COSTA_SCALED_F_ROWS;
        const int nr = frow ? t.op.nf : t.op.ns, nc = frow ? t.op.ns : t.op.nf;  // the op's rows x columns of C
        // rows [col0, col0 + nc) x columns [row0, row0 + nr) of Ct, in Ct's own coordinates
        const interval rows(rb + t.col0, rb + t.col0 + nc), cols(cb + t.row0, cb + t.row0 + nr);
        auto refuse = [&](const std::string& why) {
            return error(COSTA_ERR_ARG,
                         "costa_hip_transform_mx_dual: dual layouts: the tile of C's rows " + std::to_string(t.row0) +
                             " .. " + std::to_string(t.row0 + nr) + ", columns " + std::to_string(t.col0) + " .. " +
                             std::to_string(t.col0 + nc) + " needs rows " + std::to_string(t.col0) + " .. " +
                             std::to_string(t.col0 + nc) + " x columns " + std::to_string(t.row0) + " .. " +
                             std::to_string(t.row0 + nr) + " of Ct " + why +
                             " (Ct: C's split points and owners transposed, or coarser blocks)");
        };
        const int bi = cell_of(Ct.rows_split, rows.start), bj = cell_of(Ct.cols_split, cols.start);
        if (bi < 0 || bj < 0 || bi >= Ct.nbr() || bj >= nbc || rows.end > Ct.rows_split[size_t(bi) + 1] ||
            cols.end > Ct.cols_split[size_t(bj) + 1])
            throw refuse("inside one block, and Ct's split points cut it");
        if (Ct.owners[size_t(bi) * size_t(nbc) + size_t(bj)] != rank)
            throw refuse("on rank " + std::to_string(rank) + ", and rank " +
                         std::to_string(Ct.owners[size_t(bi) * size_t(nbc) + size_t(bj)]) + " owns that block");
        const eblock* blk = nullptr;
        const auto it = by_cell.find(int64_t(bi) * nbc + bj);
        if (it != by_cell.end())
            for (const eblock* b : it->second)
                if (b->rows.contains(rows) && b->cols.contains(cols)) blk = b;
        if (!blk) throw refuse("inside one local block, and this rank holds no such block");
        const int64_t dr = rows.start - blk->rows.start, dc = cols.start - blk->cols.start;
        const int64_t off = ct_cm ? dc * blk->ld + dr : dr * blk->ld + dc;
        if (off % g != 0)  // (a packed Ct: the op would start inside a byte / a 3-byte group)
            throw error(COSTA_ERR_ARG,
                        std::string("costa: ") + packed_rule(Ct.dtype) + ": an op starts " + std::to_string(off) +
                            " elements into its block of Ct (" + dtype_name(Ct.dtype) + "; a multiple of " +
                            std::to_string(g) + " is needed; rows " + std::to_string(t.col0) + " .., columns " +
                            std::to_string(t.row0) + " .. of Ct)");
        d.dst2 = reinterpret_cast<uintptr_t>(blk->data) + E.bytes(uint64_t(off));
        d.ldd2 = blk->ld;
        // f walks Ct's columns when it walks C's rows: contiguous in a row-major Ct (copy), strided in
        // a column-major one (transpose); the other way round when f walks C's columns
        d.flags2 = frow == ct_cm ? COSTA_TILE_TRANSPOSE : 0u;
        out.push_back(d);
    }
    return out;
}

void check_dual_ops(costa_dtype_t dst_dtype, const std::vector<costa_dual_op_t>& ops, int c_axis, int ct_axis,
                    int64_t m, int64_t n) {
    std::vector<costa_scaled_op_t> first, twin;
    first.reserve(ops.size());
    twin.reserve(ops.size());
    for (const costa_dual_op_t& t : ops) {
        first.push_back(t.s);
        twin.push_back(dual_twin_op(t));
    }
    if (c_axis >= 0) check_mx_ops(first, c_axis, m, n);
    if (ct_axis >= 0) {
        try {
            check_mx_ops(twin, ct_axis, n, m);
        } catch (const error& e) {  // (the same rule and text, naming the output it failed on)
            std::string msg = e.what();
            const std::string of_c = "MX block of C:";
            const size_t at = msg.find(of_c);
            if (at != std::string::npos) msg.replace(at, of_c.size(), "MX block of Ct (the transposed output):");
            throw error(e.code, msg);
        }
    }
    if (dtype_is_packed(dst_dtype)) {
        check_packed_ops(COSTA_FLOAT, dst_dtype, first);
        check_packed_ops(COSTA_FLOAT, dst_dtype, twin);
    }
}

void execute_tiles_mx_dual(costa_dtype_t dst_dtype, const costa_dual_op_t* ops, int64_t n_ops, const void* src_base,
                           void* dst_base, void* dst2_base, const void* scalars, int n_slots,
                           const costa_mx_scales_t* c_scales, const costa_mx_scales_t* ct_scales, int rounding,
                           int64_t m, int64_t n, const uint64_t* seed, int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const std::string who = "costa_hip_execute_tiles_mx_dual";
    if (dst_dtype == COSTA_FLOAT || !mx_pair(COSTA_FLOAT, dst_dtype))
        throw error(COSTA_ERR_ARG, who + ": no dual MX kernel for FLOAT -> " + dtype_name(dst_dtype));
    if (!c_scales || !c_scales->data) throw error(COSTA_ERR_ARG, who + ": c_scales is required");
    if (!ct_scales || !ct_scales->data) throw error(COSTA_ERR_ARG, who + ": ct_scales is required");
    if (rounding != COSTA_MX_FLOOR && rounding != COSTA_MX_CEIL)
        throw error(COSTA_ERR_ARG, who + ": rounding must be COSTA_MX_FLOOR or COSTA_MX_CEIL");
    if (m < 0 || n < 0) throw error(COSTA_ERR_ARG, who + ": negative matrix extent");
    std::vector<costa_dual_op_t> v(ops, ops + n_ops);
    std::vector<costa_scaled_op_t> first;
    for (const costa_dual_op_t& t : v) first.push_back(t.s);
    check_ops_inside(who, first, m, n);
    check_mx_scales(*c_scales, m, n, who + ": c_scales");
    check_mx_scales(*ct_scales, n, m, who + ": ct_scales");
    check_no_axpby(who, first);
    check_dual_ops(dst_dtype, v, c_scales->axis, ct_scales->axis, m, n);
    const mx_sr keys = seed ? mx_sr_keys(*seed) : mx_sr{};
    ctx(device);  // (is_device_ptr needs the device's context)
    scale_tensors_on_device(who, c_scales->data, ct_scales->data);
    const mx_side s1 = mx_side_of(*c_scales, false), s2 = mx_side_of(*ct_scales, false);
    const uintptr_t sb = reinterpret_cast<uintptr_t>(src_base), db = reinterpret_cast<uintptr_t>(dst_base),
                    db2 = reinterpret_cast<uintptr_t>(dst2_base);
    g_mx_dual_items += run_strip_tiles(
        who, v.data(), n_ops, scalars, n_slots, sizeof(float), device,
        [&](const auto& l, auto& ord, auto& w) { return build_dual_work(dst_dtype, l, sb, db, db2, ord, w, false); },
        [&](const costa_dual_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const void* d_scal, void* s) {
            launch_mx_dual(dst_dtype, d_ops, d_work, l, static_cast<const char*>(src_base),
                           static_cast<char*>(dst_base), static_cast<char*>(dst2_base), d_scal, s1, s2,
                           rounding == COSTA_MX_CEIL, s, seed ? &keys : nullptr);
        });
}

int64_t mx_dual_items(bool reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const int64_t v = g_mx_dual_items;
    if (reset) g_mx_dual_items = 0;
    return v;
}

// ---------------------------------------------------------------- block-scaled FP8 transforms
void check_block_scales(const costa_block_scales_t& s, int64_t rows, int64_t cols, const std::string& what) {
    const bool shape_ok = (s.block_rows == 1 && s.block_cols == 128) || (s.block_rows == 128 && s.block_cols == 1) ||
                          (s.block_rows == 128 && s.block_cols == 128);
    if (!shape_ok)
        throw error(COSTA_ERR_ARG, what + ": the block shape must be (1, 128), (128, 1) or (128, 128), not (" +
                                       std::to_string(s.block_rows) + ", " + std::to_string(s.block_cols) + ")");
    if (reinterpret_cast<uintptr_t>(s.data) % 4 != 0) throw error(COSTA_ERR_ARG, what + ": data must be 4-byte aligned");
    if (s.row_stride <= 0 || s.col_stride <= 0) throw error(COSTA_ERR_ARG, what + ": the strides must be positive");
    const int64_t nbr = (rows + s.block_rows - 1) / s.block_rows, nbc = (cols + s.block_cols - 1) / s.block_cols;
    // (as check_mx_scales: the smallest coincidence of two positive strides is dr = cs / g, dc = rs / g)
    if (nbr > 1 && nbc > 1) {
        const int64_t g = std::gcd(s.row_stride, s.col_stride);
        if (s.col_stride / g < nbr && s.row_stride / g < nbc)
            throw error(COSTA_ERR_ARG, what + ": the strides make two blocks share a float");
    }
}

void check_block_ops(const std::vector<costa_scaled_op_t>& ops, int block_rows, int block_cols, int64_t m,
                     int64_t n) {
    for (const costa_scaled_op_t& t : ops) {
        if (t.op.nf <= 0 || t.op.ns <= 0) continue;
        const bool frow = t.op.flags & COSTA_SCALED_F_ROWS;
        for (int rows = 1; rows >= 0; --rows) {
            const int64_t b = rows ? block_rows : block_cols;
            const int64_t at = rows ? t.row0 : t.col0, len = rows == int(frow) ? t.op.nf : t.op.ns;
            const int64_t edge = rows ? m : n;
            if (at % b != 0 || (len % b != 0 && at + len != edge) || at + len > edge)
                throw error(COSTA_ERR_ARG,
                            "costa: a tile boundary splits a scale block of C: a tile covers " +
                                std::string(rows ? "rows " : "columns ") + std::to_string(at) + " .. " +
                                std::to_string(at + len) + " of " + std::to_string(edge) +
                                " (block sizes and split points of both layouts must be multiples of " +
                                std::to_string(b) + " along " + (rows ? "rows" : "columns") + ")");
        }
    }
}

void execute_tiles_block(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, const costa_scaled_op_t* ops,
                         int64_t n_ops, const void* src_base, void* dst_base, const void* scalars, int n_slots,
                         const costa_block_scales_t* a_scales, const costa_block_scales_t* c_scales,
                         int rounding, int64_t m, int64_t n, int a_transposed, int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const std::string who = "costa_hip_execute_tiles_block_scaled";
    if (!block_pair(src_dtype, dst_dtype))
        throw error(COSTA_ERR_ARG, who + ": no block-scaled kernel for " + dtype_name(src_dtype) + " -> " +
                                       dtype_name(dst_dtype));
    const costa_block_scales_t none{};
    const costa_block_scales_t& sa = a_scales && a_scales->data ? *a_scales : none;
    const costa_block_scales_t& sc = c_scales && c_scales->data ? *c_scales : none;
    if ((sa.data != nullptr) != (src_dtype != COSTA_FLOAT) || (sc.data != nullptr) != (dst_dtype != COSTA_FLOAT))
        throw error(COSTA_ERR_ARG, who + ": a scale tensor is needed exactly on the FP8 sides of " +
                                       dtype_name(src_dtype) + " -> " + dtype_name(dst_dtype));
    if (rounding != COSTA_BLOCK_EXACT && rounding != COSTA_BLOCK_POW2)
        throw error(COSTA_ERR_ARG, who + ": rounding must be COSTA_BLOCK_EXACT or COSTA_BLOCK_POW2");
    if (m < 0 || n < 0) throw error(COSTA_ERR_ARG, who + ": negative matrix extent");
    if (sa.data) check_block_scales(sa, a_transposed ? n : m, a_transposed ? m : n, who + ": a_scales");
    std::vector<costa_scaled_op_t> v(ops, ops + n_ops);
    check_ops_inside(who, v, m, n);
    if (sc.data) {
        check_block_scales(sc, m, n, who + ": c_scales");
        check_no_axpby(who, v);
        check_block_ops(v, sc.block_rows, sc.block_cols, m, n);
    }
    ctx(device);  // (is_device_ptr needs the device's context)
    scale_tensors_on_device(who, sa.data, sc.data);
    const block_side da = block_side_of(sa, a_transposed != 0), dc_ = block_side_of(sc, false);
    const uintptr_t sb = reinterpret_cast<uintptr_t>(src_base), db = reinterpret_cast<uintptr_t>(dst_base);
    const bool quant = sc.data != nullptr;
    g_blk_items += run_strip_tiles(
        who, v.data(), n_ops, scalars, n_slots, sizeof(float), device,
        [&](const auto& l, auto& ord, auto& w) {
            return quant ? build_block_work(src_dtype, dst_dtype, l, sb, db, ord, w, false)
                         : build_scaled_work(src_dtype, dst_dtype, l, sb, db, ord, w, false);
        },
        [&](const costa_scaled_op_t* d_ops, const uint64_t* d_work, const strip_list& l, const void* d_scal, void* s) {
            launch_block(src_dtype, dst_dtype, d_ops, d_work, l, static_cast<const char*>(src_base),
                         static_cast<char*>(dst_base), d_scal, da, dc_, rounding == COSTA_BLOCK_POW2, s);
        });
}

int64_t block_items(bool reset) {
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    const int64_t v = g_blk_items;
    if (reset) g_blk_items = 0;
    return v;
}

void copy_and_transform(costa_dtype_t dtype, int n_rows, int n_cols, const void* src,
                        int src_stride, bool src_cm, void* dst, int dst_stride, bool dst_cm,
                        bool trans, bool conj, const void* alpha, const void* beta) {
    if (n_rows < 0 || n_cols < 0 || src_stride < 0 || dst_stride < 0)
        throw error(COSTA_ERR_ARG, "costa_hip_copy_and_transform: negative size or stride");
    if (dtype_is_half(dtype) || dtype_is_fp8(dtype) || dtype_is_packed(dtype))
        throw error(COSTA_ERR_ARG, std::string("costa_hip_copy_and_transform: no same-type tile kernel for ") +
                                       dtype_name(dtype));
    if (size_t(n_rows) * size_t(n_cols) == 0) return;  // memory_utils.hpp:72-74
    const size_t E = dtype_size(dtype);
    scal s;
    std::memcpy(s.alpha.data(), alpha, E);
    std::memcpy(s.beta.data(), beta, E);
    const bool cj = conj && dtype_is_complex(dtype);
    const bool wt = (trans && src_cm == dst_cm) || (!trans && src_cm != dst_cm);
    costa_tile_op_t op = make_tile_op(n_rows, n_cols, reinterpret_cast<uintptr_t>(src), src_stride,
                                      src_cm, reinterpret_cast<uintptr_t>(dst), dst_stride, dst_cm,
                                      trans, cj, scale_kind(dtype, s, !wt, cj), 0, E);
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::vector<unsigned char> sc(2 * E);
    std::memcpy(sc.data(), alpha, E);
    std::memcpy(sc.data() + E, beta, E);
    execute_tiles(dtype, &op, 1, nullptr, nullptr, sc.data(), 1, dev);
}

}  // namespace engine
}  // namespace costa
