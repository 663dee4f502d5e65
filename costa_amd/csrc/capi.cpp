// extern "C" boundary (include/costa_hip.h) and the C++ transform API
// (include/costa/transform.hpp).  No exception crosses the C boundary.
#include "engine.hpp"

#include <hip/hip_runtime.h>

#include <costa/transform.hpp>

#include <algorithm>
#include <cctype>
#include <complex>
#include <cstring>
#include <new>

struct costa_layout_s {
    costa::engine::elayout e;
    std::vector<int> base_owners;  // owners before a rank relabelling (empty: none applied)
};
struct costa_comm_s {
    costa::engine::comm* c = nullptr;
};

namespace {
thread_local std::string g_last_error;

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return COSTA_OK;
    } catch (const costa::engine::error& e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_last_error = "out of host memory";
        return COSTA_ERR_INTERNAL;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return COSTA_ERR_ARG;
    } catch (...) {
        g_last_error = "unknown error";
        return COSTA_ERR_INTERNAL;
    }
}

// Entry points that may switch the calling thread's HIP device (hipSetDevice to the
// communicator's or the call's device) put the caller's current device back on the way out:
// a process driving several GPUs keeps its own device selection across costa calls.
struct device_restore {
    int dev = -1;
    device_restore() {
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    }
    ~device_restore() {
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

template <typename F>
int gpu_guarded(F&& f) {
    device_restore keep;
    return guarded(std::forward<F>(f));
}

using costa::engine::dtype_size;
using costa::engine::elayout;
using costa::engine::job;
using costa::engine::scal;

template <typename F>
void with_type(costa_dtype_t t, F&& f) {
    switch (t) {
    case COSTA_FLOAT: f(float{}); return;
    case COSTA_DOUBLE: f(double{}); return;
    case COSTA_CFLOAT: f(std::complex<float>{}); return;
    case COSTA_CDOUBLE: f(std::complex<double>{}); return;
    case COSTA_INT32: f(int{}); return;
    case COSTA_HALF: f(costa::half_bits{}); return;
    case COSTA_BFLOAT16: f(costa::bfloat16_bits{}); return;
    case COSTA_FP8_E4M3: f(costa::fp8_e4m3_bits{}); return;
    case COSTA_FP8_E5M2: f(costa::fp8_e5m2_bits{}); return;
    // (packed: no element type of their own; packed_layout() below builds them from a byte layout)
    case COSTA_FP4_E2M1: f(costa::fp8_e4m3_bits{}); return;
    case COSTA_FP6_E2M3: f(costa::fp8_e4m3_bits{}); return;
    case COSTA_FP6_E3M2: f(costa::fp8_e4m3_bits{}); return;
    }
    throw costa::engine::error(COSTA_ERR_ARG, "unknown dtype");
}

// A packed layout (FP4_E2M1, FP6_E2M3, FP6_E3M2) from the 1-byte layout the builders made of the same
// arguments (every count in elements): the layout-only part of the type's rule -- no tile may split a
// packing group of g elements: the evenness rule, g = 2 (costa_hip.h, "MXFP4"), the quad rule, g = 4
// ("MXFP6") -- then every block pointer at the byte offset of its element offset from `base`
// (block-cyclic; a custom layout's pointers are the caller's byte pointers, base == nullptr).
// `sub_off`: the sub-matrix offset along the packed dimension (block-cyclic), else 0.
void packed_layout(elayout& e, costa_dtype_t dtype, const char* base, int sub_off) {
    const int g = costa::engine::packed_group(dtype);
    const bool fp4 = g == 2;
    auto bad = [&](const std::string& what) {
        throw costa::engine::error(COSTA_ERR_ARG, std::string("costa: ") + costa::engine::packed_rule(dtype) + ": an " +
                                                      costa::engine::dtype_name(dtype) + " layout must not split a " +
                                                      (fp4 ? "byte" : "3-byte group") + ": " + what);
    };
    const bool packed_rows = e.ordering != 'R';  // 'C': rows share bytes
    const char* dim = packed_rows ? "row" : "column";
    const std::vector<int>& split = packed_rows ? e.rows_split : e.cols_split;
    if (!split.empty() && (split.back() - split.front()) % g != 0)
        bad(std::string("the matrix has ") + std::to_string(split.back() - split.front()) + " " + dim +
            "s along the packed dimension, [" + std::to_string(split.front()) + ", " + std::to_string(split.back()) +
            ")");
    if (sub_off % g != 0)
        bad(std::string("the sub-matrix starts at ") + dim + " " + std::to_string(sub_off) + " (0-based), [" +
            std::to_string(sub_off) + ", ...)");
    for (size_t k = 0; k + 1 < split.size(); ++k)
        if (split[k] % g != 0 || split[k + 1] % g != 0)
            bad(std::string("the ") + dim + " interval [" + std::to_string(split[k]) + ", " +
                std::to_string(split[k + 1]) + ") of its own grid has an " +
                (fp4 ? "odd end" : "end that is no multiple of 4"));
    for (auto& b : e.blocks) {
        const costa::interval& iv = packed_rows ? b.rows : b.cols;
        if (b.ld % g != 0)
            bad(std::string("ld ") + std::to_string(b.ld) + " of the block at " + dim + "s [" +
                std::to_string(iv.start) + ", " + std::to_string(iv.end) + ") is " +
                (fp4 ? "odd" : "no multiple of 4"));
        if (!base) continue;
        const std::ptrdiff_t off = b.data - base;  // elements
        if (off % g != 0)
            bad(std::string("the block at ") + dim + "s [" + std::to_string(iv.start) + ", " +
                std::to_string(iv.end) + ") starts " + std::to_string(off) + " elements into the local buffer");
        b.data = const_cast<char*>(base) + costa::engine::elem_size(dtype).bytes(uint64_t(off));
    }
    e.dtype = dtype;
}

scal make_scal(costa_dtype_t t, const void* a, const void* b) {
    scal s;
    const size_t E = dtype_size(t);
    std::memcpy(s.alpha.data(), a, E);
    std::memcpy(s.beta.data(), b, E);
    return s;
}

void check_handles(int n, const costa_layout_t* A, const costa_layout_t* C) {
    if (n <= 0 || !A || !C) throw costa::engine::error(COSTA_ERR_ARG, "costa: empty batch");
    for (int i = 0; i < n; ++i)
        if (!A[i] || !C[i]) throw costa::engine::error(COSTA_ERR_ARG, "costa: null layout");
}

std::vector<job> make_jobs(int n, const costa_layout_t* A, const costa_layout_t* C,
                           const char* trans, const void* alpha, const void* beta) {
    check_handles(n, A, C);
    // alpha / beta are elements of C's type (fp32 when A or C is a 2-byte type)
    const costa_dtype_t t = costa::engine::compute_dtype(A[0]->e.dtype, C[0]->e.dtype);
    const size_t E = dtype_size(t);
    std::vector<job> jobs(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        jobs[size_t(i)].A = &A[i]->e;
        jobs[size_t(i)].C = &C[i]->e;
        jobs[size_t(i)].trans = trans ? trans[i] : 'N';
        jobs[size_t(i)].s = make_scal(t, static_cast<const char*>(alpha) + size_t(i) * E,
                                      static_cast<const char*>(beta) + size_t(i) * E);
    }
    return jobs;
}

// the one job of a triangular transform; uplo 'U' or 'L' in either case
std::vector<job> make_tri_job(costa_layout_t A, costa_layout_t C, char trans, char uplo, int k,
                              const void* alpha, const void* beta) {
    const char ul = char(std::toupper(static_cast<unsigned char>(uplo)));
    if (ul != 'U' && ul != 'L')
        throw costa::engine::error(COSTA_ERR_ARG, "costa: uplo must be 'U' or 'L'");
    auto jobs = make_jobs(1, &A, &C, &trans, alpha, beta);
    jobs[0].uplo = ul;
    jobs[0].k = k;
    return jobs;
}
}  // namespace

namespace {
// one plan (from `make`) copied out as costa_hip_plan_export documents
template <typename F>
int export_plan(F make, int n, const costa_layout_t* A, const costa_layout_t* C, const char* trans,
                const void* alpha, const void* beta, int rank, int nranks, costa_plan_info_t* info,
                costa_tile_op_t* local_ops, costa_tile_op_t* pack_ops, costa_tile_op_t* unpack_ops,
                int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                int64_t* recv_displs, void* scalars) {
    return guarded([&] {
        if (!info || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        if (nranks < 1 || rank < 0 || rank >= nranks)
            throw costa::engine::error(COSTA_ERR_ARG, "bad rank/size");
        auto jobs = make_jobs(n, A, C, trans, alpha, beta);
        std::unique_ptr<costa::engine::plan> p = make(jobs);
        info->n_local = int64_t(p->local_ops.size());
        info->n_pack = int64_t(p->pack_ops.size());
        info->n_unpack = int64_t(p->unpack_ops.size());
        info->send_elems = p->send_elems;
        info->recv_elems = p->recv_elems;
        info->local_elems = p->local_elems;
        info->n_ranks = nranks;
        info->n_slots = int32_t(p->slots.size());
        auto cp = [](const auto& v, auto* dst) {
            if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
        };
        cp(p->local_ops, local_ops);
        cp(p->pack_ops, pack_ops);
        cp(p->unpack_ops, unpack_ops);
        cp(p->send_counts, send_counts);
        cp(p->send_displs, send_displs);
        cp(p->recv_counts, recv_counts);
        cp(p->recv_displs, recv_displs);
        if (scalars) {
            const size_t E = dtype_size(p->scalar_dtype());
            auto* out = static_cast<unsigned char*>(scalars);
            for (size_t t = 0; t < p->slots.size(); ++t) {
                std::memcpy(out + (2 * t) * E, p->slots[t].alpha.data(), E);
                std::memcpy(out + (2 * t + 1) * E, p->slots[t].beta.data(), E);
            }
        }
    });
}
}  // namespace

extern "C" {

const char* costa_hip_last_error(void) { return g_last_error.c_str(); }
int costa_hip_version(void) { return 100; }

int costa_hip_device_count(int* count) {
    return guarded([&] {
        if (!count) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *count = costa::engine::device_count();
    });
}

int costa_hip_rccl_version(int* version) {
    return guarded([&] {
        if (!version) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *version = costa::engine::rccl_version();
    });
}

int costa_hip_block_cyclic_layout(costa_dtype_t dtype, int m, int n, int block_m, int block_n,
                                  int i, int j, int sub_m, int sub_n, int p_m, int p_n,
                                  char rank_grid_ordering, int rsrc, int csrc, void* ptr, int lld,
                                  char data_ordering, int rank, costa_layout_t* out) {
    return guarded([&] {
        if (!out) throw costa::engine::error(COSTA_ERR_ARG, "null output handle");
        auto h = std::make_unique<costa_layout_s>();
        with_type(dtype, [&](auto z) {
            using T = decltype(z);
            auto L = costa::block_cyclic_layout<T>(m, n, block_m, block_n, i, j, sub_m, sub_n, p_m,
                                                   p_n, rank_grid_ordering, rsrc, csrc,
                                                   static_cast<T*>(ptr), lld, data_ordering, rank);
            h->e = costa::engine::erase(L);
            if (costa::engine::dtype_is_packed(dtype))
                packed_layout(h->e, dtype, static_cast<const char*>(ptr), h->e.ordering != 'R' ? i - 1 : j - 1);
            costa::engine::set_layout_hash(h->e);  // handles are immutable
        });
        *out = h.release();
    });
}

int costa_hip_custom_layout(costa_dtype_t dtype, int rowblocks, int colblocks, const int* rowsplit,
                            const int* colsplit, const int* owners, int nlocalblocks,
                            const costa_block_t* localblocks, char ordering, costa_layout_t* out) {
    static_assert(sizeof(costa_block_t) == sizeof(costa::block_t), "block_t layout");
    return guarded([&] {
        if (!out || !rowsplit || !colsplit || !owners || (nlocalblocks > 0 && !localblocks))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto h = std::make_unique<costa_layout_s>();
        with_type(dtype, [&](auto z) {
            using T = decltype(z);
            auto L = costa::custom_layout<T>(rowblocks, colblocks, rowsplit, colsplit, owners,
                                             nlocalblocks,
                                             reinterpret_cast<const costa::block_t*>(localblocks),
                                             ordering);
            h->e = costa::engine::erase(L);
            if (costa::engine::dtype_is_packed(dtype)) packed_layout(h->e, dtype, nullptr, 0);
            costa::engine::set_layout_hash(h->e);  // handles are immutable
        });
        *out = h.release();
    });
}

void costa_hip_layout_destroy(costa_layout_t layout) { delete layout; }

int costa_hip_layout_reorder_ranks(costa_layout_t layout, const int* reordering, int n) {
    return guarded([&] {
        if (!layout || n < 0 || (n > 0 && !reordering))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto& e = layout->e;
        if (layout->base_owners.empty()) layout->base_owners = e.owners;
        const std::vector<int>& base = layout->base_owners;
        int n_base = 0;
        for (int o : base) n_base = std::max(n_base, o + 1);
        // the reference replaces the relabelling (assigned_grid2D::reorder_ranks, grid2D.hpp:219-221)
        // and maps every owner through it (owner(), grid2D.hpp:183-187)
        if (n > 0 && n < n_base)
            throw costa::engine::error(COSTA_ERR_ARG, "costa: reordering shorter than the ranks");
        std::vector<char> seen(size_t(n), 0);
        for (int k = 0; k < n; ++k) {
            if (reordering[k] < 0 || reordering[k] >= n)
                throw costa::engine::error(COSTA_ERR_ARG, "costa: reordering out of range");
            if (seen[size_t(reordering[k])]++)
                throw costa::engine::error(COSTA_ERR_ARG, "costa: reordering is not a permutation");
        }
        std::vector<int> owners(base.size());
        for (size_t k = 0; k < base.size(); ++k) owners[k] = n > 0 ? reordering[base[k]] : base[k];
        e.owners = std::move(owners);
        e.n_ranks = std::max(e.n_ranks, n);
        costa::engine::set_layout_hash(e);  // a relabelled handle is a different layout
    });
}

int costa_hip_layout_num_blocks(costa_layout_t layout) {
    return layout ? int(layout->e.blocks.size()) : -1;
}

int costa_hip_layout_shape(costa_layout_t layout, int* m, int* n) {
    return guarded([&] {
        if (!layout || !m || !n) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        const auto& e = layout->e;
        *m = e.rows_split.empty() ? 0 : e.rows_split.back() - e.rows_split.front();
        *n = e.cols_split.empty() ? 0 : e.cols_split.back() - e.cols_split.front();
    });
}

int costa_hip_layout_block(costa_layout_t layout, int i, int* row_start, int* row_end,
                           int* col_start, int* col_end, void** data, int* ld) {
    return guarded([&] {
        if (!layout || i < 0 || size_t(i) >= layout->e.blocks.size())
            throw costa::engine::error(COSTA_ERR_ARG, "block index out of range");
        const auto& b = layout->e.blocks[size_t(i)];
        if (row_start) *row_start = b.rows.start;
        if (row_end) *row_end = b.rows.end;
        if (col_start) *col_start = b.cols.start;
        if (col_end) *col_end = b.cols.end;
        if (data) *data = b.data;
        if (ld) *ld = b.ld;
    });
}

int costa_hip_comm_self(int device, costa_comm_t* out) {
    return gpu_guarded([&] {
        if (!out) throw costa::engine::error(COSTA_ERR_ARG, "null output handle");
        auto h = std::make_unique<costa_comm_s>();
        h->c = costa::engine::comm_self(device);
        *out = h.release();
    });
}

int costa_hip_comm_unique_id(unsigned char id[128]) {
    return guarded([&] { costa::engine::comm_unique_id(id); });
}

int costa_hip_comm_create(const unsigned char id[128], int nranks, int rank, int device,
                          costa_comm_t* out) {
    return gpu_guarded([&] {
        if (!out || !id) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto h = std::make_unique<costa_comm_s>();
        h->c = costa::engine::comm_create(id, nranks, rank, device);
        *out = h.release();
    });
}

int costa_hip_comm_emulated(int rank, int nranks, int device, costa_comm_t* out) {
    return gpu_guarded([&] {
        if (!out) throw costa::engine::error(COSTA_ERR_ARG, "null output handle");
        auto h = std::make_unique<costa_comm_s>();
        h->c = costa::engine::comm_emulated(rank, nranks, device);
        *out = h.release();
    });
}

int costa_hip_comm_emulate(costa_comm_t comm, int part, int round, void* buffer) {
    return gpu_guarded([&] {
        if (!comm) throw costa::engine::error(COSTA_ERR_ARG, "null communicator");
        costa::engine::comm_emulate(comm->c, part, round, buffer);
    });
}

int costa_hip_exchange_rounds(void) { return costa::engine::exchange_rounds(); }

int costa_hip_round_range(int64_t count, int elem_bytes, int rounds, int round, int64_t* lo,
                          int64_t* hi) {
    return guarded([&] {
        if (!lo || !hi) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        if (count < 0 || elem_bytes < 1 || rounds < 1 || round < 0)
            throw costa::engine::error(COSTA_ERR_ARG, "costa_hip_round_range: negative count or round, "
                                                      "or no element size or rounds");
        costa::engine::round_range(count, size_t(elem_bytes), rounds, round, *lo, *hi);
    });
}

int costa_hip_comm_rank(costa_comm_t comm) { return comm ? costa::engine::comm_rank(comm->c) : -1; }
int costa_hip_comm_size(costa_comm_t comm) { return comm ? costa::engine::comm_size(comm->c) : -1; }
void costa_hip_comm_destroy(costa_comm_t comm) {
    if (!comm) return;
    costa::engine::comm_destroy(comm->c);
    delete comm;
}

int costa_hip_transform(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                        const void* beta, costa_comm_t comm) {
    return costa_hip_transform_batch(1, &A, &C, &trans, alpha, beta, comm);
}

int costa_hip_transform_batch(int n, const costa_layout_t* A, const costa_layout_t* C,
                              const char* trans, const void* alpha, const void* beta,
                              costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_jobs(n, A, C, trans, alpha, beta);
        costa::engine::transform(jobs, comm->c);
    });
}

int costa_hip_transform_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                              const void* beta, costa_comm_t comm, void* stream) {
    return costa_hip_transform_batch_async(1, &A, &C, &trans, alpha, beta, comm, stream);
}

int costa_hip_transform_batch_async(int n, const costa_layout_t* A, const costa_layout_t* C,
                                    const char* trans, const void* alpha, const void* beta,
                                    costa_comm_t comm, void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_jobs(n, A, C, trans, alpha, beta);
        costa::engine::transform(jobs, comm->c, stream, true);
    });
}

int costa_hip_transform_tri(costa_layout_t A, costa_layout_t C, char trans, char uplo, int k,
                            const void* alpha, const void* beta, costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_tri_job(A, C, trans, uplo, k, alpha, beta), comm->c);
    });
}

int costa_hip_transform_tri_async(costa_layout_t A, costa_layout_t C, char trans, char uplo, int k,
                                  const void* alpha, const void* beta, costa_comm_t comm,
                                  void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_tri_job(A, C, trans, uplo, k, alpha, beta), comm->c, stream, true);
    });
}

int costa_hip_execute_tiles_tri(costa_dtype_t dtype, const costa_tri_op_t* ops, int64_t n,
                                const void* src_base, void* dst_base, const void* scalars,
                                int n_slots, int device) {
    static_assert(sizeof(costa_tile_op_t) == 40 && sizeof(costa_tri_op_t) == 48, "descriptor sizes");
    return gpu_guarded([&] {
        if (n < 0 || (n > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_tri(dtype, ops, n, src_base, dst_base, scalars, n_slots, device);
    });
}

int costa_hip_tri_cut(void) { return costa::engine::kTriCut; }

int costa_hip_tri_phase_ms(double* ms, int reset) {
    return guarded([&] {
        if (!ms) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *ms = costa::engine::tri_phase_ms(reset != 0);
    });
}

int costa_hip_tri_subtile(costa_dtype_t dtype, int* bf, int* bs) {
    return guarded([&] {
        if (!bf || !bs) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::tri_subtile(dtype, bf, bs);
    });
}

int costa_hip_plan_export_tri(costa_layout_t A, costa_layout_t C, char trans, char uplo, int k,
                              const void* alpha, const void* beta, int rank, int nranks,
                              costa_tri_plan_info_t* info, costa_tile_op_t* local_ops,
                              costa_tile_op_t* pack_ops, costa_tile_op_t* unpack_ops,
                              costa_tri_op_t* local_tri, costa_tri_op_t* unpack_tri,
                              int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                              int64_t* recv_displs, void* scalars) {
    return guarded([&] {
        if (!info || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        if (nranks < 1 || rank < 0 || rank >= nranks)
            throw costa::engine::error(COSTA_ERR_ARG, "bad rank/size");
        check_handles(1, &A, &C);
        auto p = costa::engine::make_plan(make_tri_job(A, C, trans, uplo, k, alpha, beta), rank, nranks);
        info->base.n_local = int64_t(p->local_ops.size());
        info->base.n_pack = int64_t(p->pack_ops.size());
        info->base.n_unpack = int64_t(p->unpack_ops.size());
        info->base.send_elems = p->send_elems;
        info->base.recv_elems = p->recv_elems;
        info->base.local_elems = p->local_elems;
        info->base.n_ranks = nranks;
        info->base.n_slots = int32_t(p->slots.size());
        info->n_local_tri = int64_t(p->local_tri.size());
        info->n_unpack_tri = int64_t(p->unpack_tri.size());
        auto cp = [](const auto& v, auto* dst) {
            if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
        };
        cp(p->local_ops, local_ops);
        cp(p->pack_ops, pack_ops);
        cp(p->unpack_ops, unpack_ops);
        cp(p->local_tri, local_tri);
        cp(p->unpack_tri, unpack_tri);
        cp(p->send_counts, send_counts);
        cp(p->send_displs, send_displs);
        cp(p->recv_counts, recv_counts);
        cp(p->recv_displs, recv_displs);
        if (scalars) {
            const size_t E = dtype_size(p->dtype);
            auto* out = static_cast<unsigned char*>(scalars);
            std::memcpy(out, p->slots[0].alpha.data(), E);
            std::memcpy(out + E, p->slots[0].beta.data(), E);
        }
    });
}

namespace {
// the one job of a scaled transform
std::vector<job> make_scaled_job(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                 const void* beta, const void* row_scale, const void* col_scale) {
    auto jobs = make_jobs(1, &A, &C, &trans, alpha, beta);
    jobs[0].scaled = true;
    jobs[0].row_scale = row_scale;
    jobs[0].col_scale = col_scale;
    return jobs;
}
void check_scale_vectors(const void* row_scale, const void* col_scale) {
    if (!row_scale && !col_scale)
        throw costa::engine::error(COSTA_ERR_ARG, "costa_hip_transform_scaled: both scale vectors are "
                                                  "NULL (use costa_hip_transform)");
}
}  // namespace

int costa_hip_transform_scaled(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                               const void* beta, const void* row_scale, const void* col_scale,
                               costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_scaled_job(A, C, trans, alpha, beta, row_scale, col_scale);
        costa_dtype_t a, c;  // an unsupported pair is reported first
        costa::engine::check_jobs(jobs, costa::engine::comm_size(comm->c), a, c);
        check_scale_vectors(row_scale, col_scale);
        costa::engine::transform(jobs, comm->c);
    });
}

int costa_hip_transform_scaled_async(costa_layout_t A, costa_layout_t C, char trans,
                                     const void* alpha, const void* beta, const void* row_scale,
                                     const void* col_scale, costa_comm_t comm, void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_scaled_job(A, C, trans, alpha, beta, row_scale, col_scale);
        costa_dtype_t a, c;
        costa::engine::check_jobs(jobs, costa::engine::comm_size(comm->c), a, c);
        check_scale_vectors(row_scale, col_scale);
        costa::engine::transform(jobs, comm->c, stream, true);
    });
}

int costa_hip_execute_tiles_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                   const costa_scaled_op_t* ops, int64_t n, const void* src_base,
                                   void* dst_base, const void* scalars, int n_slots,
                                   const void* row_scale, const void* col_scale, int device) {
    static_assert(sizeof(costa_scaled_op_t) == 48, "descriptor size");
    return gpu_guarded([&] {
        if (n < 0 || (n > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_scaled(src_dtype, dst_dtype, ops, n, src_base, dst_base, scalars,
                                            n_slots, row_scale, col_scale, device);
    });
}

int costa_hip_scaled_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs) {
    return guarded([&] {
        if (!bf || !bs) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::scaled_subtile(src_dtype, dst_dtype, bf, bs);
    });
}

int costa_hip_mx_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs) {
    return guarded([&] {
        if (!bf || !bs) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::mx_subtile(src_dtype, dst_dtype, bf, bs);
    });
}

int costa_hip_block_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs) {
    return guarded([&] {
        if (!bf || !bs) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::block_subtile(src_dtype, dst_dtype, bf, bs);
    });
}

int costa_hip_scaled_items(int64_t* items, int reset) {
    return guarded([&] {
        if (!items) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *items = costa::engine::scaled_items(reset != 0);
    });
}

namespace {
// the one job of costa_hip_transform_amax: a scaled job (the scaled plan, unchanged) with outputs
std::vector<job> make_amax_job(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                               const void* beta, const void* row_scale, const void* col_scale,
                               void* row_amax, void* col_amax) {
    auto jobs = make_scaled_job(A, C, trans, alpha, beta, row_scale, col_scale);
    jobs[0].row_amax = row_amax;
    jobs[0].col_amax = col_amax;
    return jobs;
}
void check_amax_vectors(const void* row_amax, const void* col_amax) {
    if (!row_amax && !col_amax)
        throw costa::engine::error(COSTA_ERR_ARG, "costa_hip_transform_amax: both amax vectors are NULL (use "
                                                  "costa_hip_transform_scaled or costa_hip_transform)");
}
}  // namespace

int costa_hip_transform_amax(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                             const void* beta, const void* row_scale, const void* col_scale,
                             void* row_amax, void* col_amax, costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_amax_job(A, C, trans, alpha, beta, row_scale, col_scale, row_amax, col_amax);
        costa_dtype_t a, c;  // an unsupported pair is reported first
        costa::engine::check_jobs(jobs, costa::engine::comm_size(comm->c), a, c);
        check_amax_vectors(row_amax, col_amax);
        costa::engine::transform(jobs, comm->c);
    });
}

int costa_hip_transform_amax_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                   const void* beta, const void* row_scale, const void* col_scale,
                                   void* row_amax, void* col_amax, costa_comm_t comm, void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_amax_job(A, C, trans, alpha, beta, row_scale, col_scale, row_amax, col_amax);
        costa_dtype_t a, c;
        costa::engine::check_jobs(jobs, costa::engine::comm_size(comm->c), a, c);
        check_amax_vectors(row_amax, col_amax);
        costa::engine::transform(jobs, comm->c, stream, true);
    });
}

int costa_hip_layout_amax(costa_layout_t A, void* row_amax, void* col_amax, costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!A || !comm) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::layout_amax(A->e, row_amax, col_amax, comm->c, nullptr, false);
    });
}

int costa_hip_layout_amax_async(costa_layout_t A, void* row_amax, void* col_amax, costa_comm_t comm,
                                void* stream) {
    return gpu_guarded([&] {
        if (!A || !comm) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::layout_amax(A->e, row_amax, col_amax, comm->c, stream, true);
    });
}

int costa_hip_execute_tiles_amax(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                 const costa_scaled_op_t* ops, int64_t n, const void* src_base,
                                 void* dst_base, const void* scalars, int n_slots, const void* row_scale,
                                 const void* col_scale, void* row_amax, void* col_amax, int device) {
    return gpu_guarded([&] {
        if (n < 0 || (n > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_amax(src_dtype, dst_dtype, ops, n, src_base, dst_base, scalars,
                                          n_slots, row_scale, col_scale, row_amax, col_amax, device);
    });
}

int costa_hip_amax_items(int64_t* items, int reset) {
    return guarded([&] {
        if (!items) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *items = costa::engine::amax_items(reset != 0);
    });
}

namespace {
// the one job of costa_hip_transform_mx: a scaled job (the scaled plan, unchanged) whose lists run on
// mx_kernel; an absent descriptor (NULL, or NULL data) is all zeros
std::vector<job> make_mx_job(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                             const void* beta, const costa_mx_scales_t* a_scales,
                             const costa_mx_scales_t* c_scales, int rounding) {
    auto jobs = make_scaled_job(A, C, trans, alpha, beta, nullptr, nullptr);
    jobs[0].mx = true;
    if (a_scales && a_scales->data) jobs[0].a_scales = *a_scales;
    if (c_scales && c_scales->data) jobs[0].c_scales = *c_scales;
    jobs[0].mx_rounding = rounding;
    return jobs;
}
}  // namespace

int costa_hip_transform_mx(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                           const void* beta, const costa_mx_scales_t* a_scales,
                           const costa_mx_scales_t* c_scales, int rounding, costa_comm_t comm) {
    static_assert(sizeof(costa_mx_scales_t) == 32, "descriptor size");
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_mx_job(A, C, trans, alpha, beta, a_scales, c_scales, rounding), comm->c);
    });
}

int costa_hip_transform_mx_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                 const void* beta, const costa_mx_scales_t* a_scales,
                                 const costa_mx_scales_t* c_scales, int rounding, costa_comm_t comm,
                                 void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_mx_job(A, C, trans, alpha, beta, a_scales, c_scales, rounding), comm->c,
                                 stream, true);
    });
}

int costa_hip_execute_tiles_mx(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                               const costa_scaled_op_t* ops, int64_t n_ops, const void* src_base,
                               void* dst_base, const void* scalars, int n_slots,
                               const costa_mx_scales_t* a_scales, const costa_mx_scales_t* c_scales,
                               int rounding, int64_t m, int64_t n, int a_transposed, int device) {
    return gpu_guarded([&] {
        if (n_ops < 0 || (n_ops > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_mx(src_dtype, dst_dtype, ops, n_ops, src_base, dst_base, scalars, n_slots,
                                        a_scales, c_scales, rounding, m, n, a_transposed, device);
    });
}

int costa_hip_transform_mx_sr(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                              const void* beta, const costa_mx_scales_t* a_scales,
                              const costa_mx_scales_t* c_scales, int rounding, uint64_t seed,
                              costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_mx_job(A, C, trans, alpha, beta, a_scales, c_scales, rounding);
        jobs[0].mx_sr = true;
        jobs[0].mx_seed = seed;
        costa::engine::transform(jobs, comm->c);
    });
}

int costa_hip_transform_mx_sr_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                    const void* beta, const costa_mx_scales_t* a_scales,
                                    const costa_mx_scales_t* c_scales, int rounding, uint64_t seed,
                                    costa_comm_t comm, void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        auto jobs = make_mx_job(A, C, trans, alpha, beta, a_scales, c_scales, rounding);
        jobs[0].mx_sr = true;
        jobs[0].mx_seed = seed;
        costa::engine::transform(jobs, comm->c, stream, true);
    });
}

int costa_hip_execute_tiles_mx_sr(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                  const costa_scaled_op_t* ops, int64_t n_ops, const void* src_base,
                                  void* dst_base, const void* scalars, int n_slots,
                                  const costa_mx_scales_t* a_scales, const costa_mx_scales_t* c_scales,
                                  int rounding, int64_t m, int64_t n, int a_transposed, uint64_t seed,
                                  int device) {
    return gpu_guarded([&] {
        if (n_ops < 0 || (n_ops > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_mx(src_dtype, dst_dtype, ops, n_ops, src_base, dst_base, scalars, n_slots,
                                        a_scales, c_scales, rounding, m, n, a_transposed, device, &seed);
    });
}

int costa_hip_sr_bits(uint64_t seed, int64_t i, int64_t j, uint32_t* u24) {
    return guarded([&] {
        if (!u24) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *u24 = costa::engine::mx_sr_bits(seed, i, j);
    });
}

int costa_hip_mx_items(int64_t* items, int reset) {
    return guarded([&] {
        if (!items) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *items = costa::engine::mx_items(reset != 0);
    });
}

namespace {
// the one job of costa_hip_transform_mx_dual: the MX job of (A, C, trans) with beta = 0, plus the second
// target and its descriptor
std::vector<job> make_dual_job(costa_layout_t A, costa_layout_t C, costa_layout_t Ct, char trans, const void* alpha,
                               const costa_mx_scales_t* c_scales, const costa_mx_scales_t* ct_scales, int rounding,
                               const uint64_t* sr_seed) {
    static_assert(sizeof(costa_dual_op_t) == 64, "dual op size");
    if (!Ct) throw costa::engine::error(COSTA_ERR_ARG, "costa: null layout");
    check_handles(1, &A, &C);
    const float beta = 0.0f;
    // (A's type is checked by the call itself: a non-FLOAT A must not reach the scaled job's pair table)
    if (A->e.dtype != COSTA_FLOAT)
        throw costa::engine::error(COSTA_ERR_ARG,
                                   std::string("costa_hip_transform_mx_dual: A must be COSTA_FLOAT, not ") +
                                       costa::engine::dtype_name(A->e.dtype) +
                                       " (no dual MX transform from a quantised or half source)");
    if (C->e.dtype != Ct->e.dtype || C->e.dtype == COSTA_FLOAT || !costa::engine::mx_pair(COSTA_FLOAT, C->e.dtype))
        throw costa::engine::error(COSTA_ERR_ARG,
                                   std::string("costa_hip_transform_mx_dual: no dual MX transform for FLOAT -> ") +
                                       costa::engine::dtype_name(C->e.dtype) + " / " +
                                       costa::engine::dtype_name(Ct->e.dtype) +
                                       " (C and Ct of one type: FP8_E4M3, FP8_E5M2, FP4_E2M1, FP6_E2M3 or FP6_E3M2)");
    auto jobs = make_mx_job(A, C, trans, alpha, &beta, nullptr, c_scales, rounding);
    jobs[0].Ct = &Ct->e;
    if (ct_scales && ct_scales->data) jobs[0].ct_scales = *ct_scales;
    if (sr_seed) {
        jobs[0].mx_sr = true;
        jobs[0].mx_seed = *sr_seed;
    }
    return jobs;
}
}  // namespace

int costa_hip_transform_mx_dual(costa_layout_t A, costa_layout_t C, costa_layout_t Ct, char trans,
                                const void* alpha, const costa_mx_scales_t* c_scales,
                                const costa_mx_scales_t* ct_scales, int rounding, const uint64_t* sr_seed,
                                costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!comm || !alpha) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_dual_job(A, C, Ct, trans, alpha, c_scales, ct_scales, rounding, sr_seed), comm->c);
    });
}

int costa_hip_transform_mx_dual_async(costa_layout_t A, costa_layout_t C, costa_layout_t Ct, char trans,
                                      const void* alpha, const costa_mx_scales_t* c_scales,
                                      const costa_mx_scales_t* ct_scales, int rounding,
                                      const uint64_t* sr_seed, costa_comm_t comm, void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_dual_job(A, C, Ct, trans, alpha, c_scales, ct_scales, rounding, sr_seed), comm->c,
                                 stream, true);
    });
}

int costa_hip_execute_tiles_mx_dual(costa_dtype_t dst_dtype, const costa_dual_op_t* ops, int64_t n_ops,
                                    const void* src_base, void* dst_base, void* dst2_base,
                                    const void* scalars, int n_slots, const costa_mx_scales_t* c_scales,
                                    const costa_mx_scales_t* ct_scales, int rounding, int64_t m, int64_t n,
                                    const uint64_t* sr_seed, int device) {
    return gpu_guarded([&] {
        if (n_ops < 0 || (n_ops > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_mx_dual(dst_dtype, ops, n_ops, src_base, dst_base, dst2_base, scalars, n_slots,
                                             c_scales, ct_scales, rounding, m, n, sr_seed, device);
    });
}

int costa_hip_mx_dual_items(int64_t* items, int reset) {
    return guarded([&] {
        if (!items) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *items = costa::engine::mx_dual_items(reset != 0);
    });
}

int costa_hip_plan_export_dual(costa_layout_t A, costa_layout_t C, costa_layout_t Ct, char trans,
                               const void* alpha, int c_axis, int ct_axis, int rank, int nranks,
                               costa_scaled_plan_info_t* info, costa_dual_op_t* local_dual,
                               costa_dual_op_t* unpack_dual) {
    return guarded([&] {
        if (!info || !alpha) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        if (nranks < 1 || rank < 0 || rank >= nranks)
            throw costa::engine::error(COSTA_ERR_ARG, "bad rank/size");
        for (int ax : {c_axis, ct_axis})
            if (ax != -1 && ax != COSTA_MX_ROWS && ax != COSTA_MX_COLS)
                throw costa::engine::error(COSTA_ERR_ARG, "costa_hip_plan_export_dual: an axis must be COSTA_MX_ROWS, "
                                                          "COSTA_MX_COLS or -1");
        auto jobs = make_dual_job(A, C, Ct, trans, alpha, nullptr, nullptr, COSTA_MX_FLOOR, nullptr);
        int64_t m = 0, n = 0, r = 0, k = 0;
        if (!C->e.rows_split.empty() && !C->e.cols_split.empty()) {
            m = int64_t(C->e.rows_split.back()) - C->e.rows_split.front();
            n = int64_t(C->e.cols_split.back()) - C->e.cols_split.front();
        }
        if (!Ct->e.rows_split.empty() && !Ct->e.cols_split.empty()) {
            r = int64_t(Ct->e.rows_split.back()) - Ct->e.rows_split.front();
            k = int64_t(Ct->e.cols_split.back()) - Ct->e.cols_split.front();
        }
        if (Ct == A || Ct == C)
            throw costa::engine::error(COSTA_ERR_ARG, "costa_hip_plan_export_dual: Ct must be a layout of its own");
        if (r != n || k != m)
            throw costa::engine::error(COSTA_ERR_ARG,
                                       "costa_hip_plan_export_dual: dual layouts: Ct describes a " + std::to_string(r) +
                                           " x " + std::to_string(k) + " matrix, the transpose of C's " +
                                           std::to_string(m) + " x " + std::to_string(n) + " is " + std::to_string(n) +
                                           " x " + std::to_string(m));
        auto p = costa::engine::make_plan(jobs, rank, nranks);
        const auto ld = costa::engine::dual_twins(p->local_scaled, Ct->e, rank);
        const auto ud = costa::engine::dual_twins(p->unpack_scaled, Ct->e, rank);
        costa::engine::check_dual_ops(C->e.dtype, ld, c_axis, ct_axis, m, n);
        costa::engine::check_dual_ops(C->e.dtype, ud, c_axis, ct_axis, m, n);
        *info = costa_scaled_plan_info_t{};
        info->base.n_pack = int64_t(p->pack_ops.size());
        info->base.send_elems = p->send_elems;
        info->base.recv_elems = p->recv_elems;
        info->base.local_elems = p->local_elems;
        info->base.n_ranks = nranks;
        info->base.n_slots = int32_t(p->slots.size());
        info->n_local_scaled = int64_t(ld.size());
        info->n_unpack_scaled = int64_t(ud.size());
        if (local_dual && !ld.empty()) std::memcpy(local_dual, ld.data(), ld.size() * sizeof(ld[0]));
        if (unpack_dual && !ud.empty()) std::memcpy(unpack_dual, ud.data(), ud.size() * sizeof(ud[0]));
    });
}

int costa_hip_mx_check_ops(const costa_scaled_op_t* ops, int64_t n_ops, int axis, int64_t m, int64_t n) {
    return guarded([&] {
        if (n_ops < 0 || (n_ops > 0 && !ops)) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        if (axis != COSTA_MX_ROWS && axis != COSTA_MX_COLS)
            throw costa::engine::error(COSTA_ERR_ARG, "costa_hip_mx_check_ops: axis must be COSTA_MX_ROWS or "
                                                      "COSTA_MX_COLS");
        costa::engine::check_mx_ops(std::vector<costa_scaled_op_t>(ops, ops + n_ops), axis, m, n);
    });
}

int costa_hip_mx_check_scales(const costa_mx_scales_t* s, int64_t rows, int64_t cols) {
    return guarded([&] {
        if (!s) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::check_mx_scales(*s, rows, cols, "costa_hip_mx_check_scales");
    });
}

namespace {
// the one job of costa_hip_transform_block_scaled: a scaled job (the scaled plan, unchanged) whose
// lists run on block_kernel; an absent descriptor (NULL, or NULL data) is all zeros
std::vector<job> make_block_job(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                const void* beta, const costa_block_scales_t* a_scales,
                                const costa_block_scales_t* c_scales, int rounding) {
    check_handles(1, &A, &C);
    const costa_dtype_t a = A->e.dtype, c = C->e.dtype;
    if (!costa::engine::block_pair(a, c))  // (before the scaled job's own pair check)
        throw costa::engine::error(COSTA_ERR_ARG,
                                   std::string("costa_hip_transform_block_scaled: no block-scaled transform for ") +
                                       costa::engine::dtype_name(a) + " -> " + costa::engine::dtype_name(c) +
                                       " (FLOAT -> FP8, FP8 -> FLOAT, FP8 -> the same FP8)");
    auto jobs = make_scaled_job(A, C, trans, alpha, beta, nullptr, nullptr);
    jobs[0].blk = true;
    if (a_scales && a_scales->data) jobs[0].a_blocks = *a_scales;
    if (c_scales && c_scales->data) jobs[0].c_blocks = *c_scales;
    jobs[0].blk_rounding = rounding;
    return jobs;
}
}  // namespace

int costa_hip_transform_block_scaled(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                     const void* beta, const costa_block_scales_t* a_scales,
                                     const costa_block_scales_t* c_scales, int rounding, costa_comm_t comm) {
    static_assert(sizeof(costa_block_scales_t) == 32, "descriptor size");
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_block_job(A, C, trans, alpha, beta, a_scales, c_scales, rounding), comm->c);
    });
}

int costa_hip_transform_block_scaled_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                           const void* beta, const costa_block_scales_t* a_scales,
                                           const costa_block_scales_t* c_scales, int rounding,
                                           costa_comm_t comm, void* stream) {
    return gpu_guarded([&] {
        if (!comm || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::transform(make_block_job(A, C, trans, alpha, beta, a_scales, c_scales, rounding), comm->c,
                                 stream, true);
    });
}

int costa_hip_execute_tiles_block_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                         const costa_scaled_op_t* ops, int64_t n_ops, const void* src_base,
                                         void* dst_base, const void* scalars, int n_slots,
                                         const costa_block_scales_t* a_scales,
                                         const costa_block_scales_t* c_scales, int rounding, int64_t m,
                                         int64_t n, int a_transposed, int device) {
    return gpu_guarded([&] {
        if (n_ops < 0 || (n_ops > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_block(src_dtype, dst_dtype, ops, n_ops, src_base, dst_base, scalars, n_slots,
                                           a_scales, c_scales, rounding, m, n, a_transposed, device);
    });
}

int costa_hip_block_items(int64_t* items, int reset) {
    return guarded([&] {
        if (!items) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        *items = costa::engine::block_items(reset != 0);
    });
}

int costa_hip_block_check_ops(const costa_scaled_op_t* ops, int64_t n_ops, int block_rows, int block_cols,
                              int64_t m, int64_t n) {
    return guarded([&] {
        if (n_ops < 0 || (n_ops > 0 && !ops)) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa_block_scales_t shape{};
        shape.block_rows = block_rows;
        shape.block_cols = block_cols;
        shape.row_stride = shape.col_stride = 1;
        costa::engine::check_block_scales(shape, 1, 1, "costa_hip_block_check_ops");  // (the block shape)
        costa::engine::check_block_ops(std::vector<costa_scaled_op_t>(ops, ops + n_ops), block_rows, block_cols, m, n);
    });
}

int costa_hip_block_check_scales(const costa_block_scales_t* desc, int64_t rows, int64_t cols) {
    return guarded([&] {
        if (!desc) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::check_block_scales(*desc, rows, cols, "costa_hip_block_check_scales");
    });
}

int costa_hip_plan_export_scaled(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                 const void* beta, int rank, int nranks,
                                 costa_scaled_plan_info_t* info, costa_tile_op_t* pack_ops,
                                 costa_scaled_op_t* local_scaled, costa_scaled_op_t* unpack_scaled,
                                 int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                                 int64_t* recv_displs, void* scalars) {
    return guarded([&] {
        if (!info || !alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        if (nranks < 1 || rank < 0 || rank >= nranks)
            throw costa::engine::error(COSTA_ERR_ARG, "bad rank/size");
        check_handles(1, &A, &C);
        auto jobs = make_scaled_job(A, C, trans, alpha, beta, nullptr, nullptr);
        // (a packed pair has a scaled plan as an MX job only: costa_hip.h, "MXFP4", "MXFP6")
        if (costa::engine::dtype_is_packed(A->e.dtype) || costa::engine::dtype_is_packed(C->e.dtype)) jobs[0].mx = true;
        auto p = costa::engine::make_plan(jobs, rank, nranks);
        info->base.n_local = int64_t(p->local_ops.size());
        info->base.n_pack = int64_t(p->pack_ops.size());
        info->base.n_unpack = int64_t(p->unpack_ops.size());
        info->base.send_elems = p->send_elems;
        info->base.recv_elems = p->recv_elems;
        info->base.local_elems = p->local_elems;
        info->base.n_ranks = nranks;
        info->base.n_slots = int32_t(p->slots.size());
        info->n_local_scaled = int64_t(p->local_scaled.size());
        info->n_unpack_scaled = int64_t(p->unpack_scaled.size());
        auto cp = [](const auto& v, auto* dst) {
            if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
        };
        cp(p->pack_ops, pack_ops);
        cp(p->local_scaled, local_scaled);
        cp(p->unpack_scaled, unpack_scaled);
        cp(p->send_counts, send_counts);
        cp(p->send_displs, send_displs);
        cp(p->recv_counts, recv_counts);
        cp(p->recv_displs, recv_displs);
        if (scalars) {
            const size_t E = dtype_size(p->scalar_dtype());
            auto* out = static_cast<unsigned char*>(scalars);
            std::memcpy(out, p->slots[0].alpha.data(), E);
            std::memcpy(out + E, p->slots[0].beta.data(), E);
        }
    });
}

int costa_hip_synchronize(costa_comm_t comm) {
    return gpu_guarded([&] {
        if (!comm) throw costa::engine::error(COSTA_ERR_ARG, "null communicator");
        costa::engine::synchronize(comm->c);
    });
}

int costa_hip_copy_and_transform(costa_dtype_t dtype, int n_rows, int n_cols, const void* src,
                                 int src_stride, int src_col_major, void* dst, int dst_stride,
                                 int dst_col_major, int transpose, int conjugate,
                                 const void* alpha, const void* beta) {
    return gpu_guarded([&] {
        if (!alpha || !beta) throw costa::engine::error(COSTA_ERR_ARG, "null scalar");
        costa::engine::copy_and_transform(dtype, n_rows, n_cols, src, src_stride, src_col_major != 0,
                                          dst, dst_stride, dst_col_major != 0, transpose != 0,
                                          conjugate != 0, alpha, beta);
    });
}

int costa_hip_execute_tiles(costa_dtype_t dtype, const costa_tile_op_t* ops, int64_t n,
                            const void* src_base, void* dst_base, const void* scalars,
                            int n_slots, int device) {
    return gpu_guarded([&] {
        if (n < 0 || (n > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles(dtype, ops, n, src_base, dst_base, scalars, n_slots, device);
    });
}

int costa_hip_execute_tiles_mixed(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                  const costa_tile_op_t* ops, int64_t n, const void* src_base,
                                  void* dst_base, const void* scalars, int n_slots, int device) {
    return gpu_guarded([&] {
        if (n < 0 || (n > 0 && (!ops || !scalars)))
            throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::execute_tiles_mixed(src_dtype, dst_dtype, ops, n, src_base, dst_base, scalars,
                                           n_slots, device);
    });
}

int costa_hip_convert_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs) {
    return guarded([&] {
        if (!bf || !bs) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::convert_subtile(src_dtype, dst_dtype, bf, bs);
    });
}

int costa_hip_plan_export(int n, const costa_layout_t* A, const costa_layout_t* C,
                          const char* trans, const void* alpha, const void* beta, int rank,
                          int nranks, costa_plan_info_t* info, costa_tile_op_t* local_ops,
                          costa_tile_op_t* pack_ops, costa_tile_op_t* unpack_ops,
                          int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                          int64_t* recv_displs, void* scalars) {
    return export_plan(
        [&](const std::vector<job>& jobs) { return costa::engine::make_plan(jobs, rank, nranks); },
        n, A, C, trans, alpha, beta, rank, nranks, info, local_ops, pack_ops, unpack_ops,
        send_counts, send_displs, recv_counts, recv_displs, scalars);
}

int costa_hip_plan_export_device(int device, int n, const costa_layout_t* A, const costa_layout_t* C,
                                 const char* trans, const void* alpha, const void* beta, int rank,
                                 int nranks, costa_plan_info_t* info, costa_tile_op_t* local_ops,
                                 costa_tile_op_t* pack_ops, costa_tile_op_t* unpack_ops,
                                 int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                                 int64_t* recv_displs, void* scalars) {
    device_restore keep;
    return export_plan(
        [&](const std::vector<job>& jobs) {
            auto p = costa::engine::make_plan_device(jobs, rank, nranks, 0, device, nullptr);
            if (!p)
                throw costa::engine::error(COSTA_ERR_ARG,
                                           "costa: the device planner does not apply to these "
                                           "layouts (local blocks are not exactly the rank's grid "
                                           "cells)");
            return p;
        },
        n, A, C, trans, alpha, beta, rank, nranks, info, local_ops, pack_ops, unpack_ops,
        send_counts, send_displs, recv_counts, recv_displs, scalars);
}

int costa_hip_set_planner(int mode) {
    return guarded([&] {
        if (mode < 0 || mode > 2) throw costa::engine::error(COSTA_ERR_ARG, "mode must be 0, 1 or 2");
        costa::engine::set_planner_mode(mode);
    });
}

int costa_hip_set_list_builder(int mode) {
    return guarded([&] {
        if (mode < 0 || mode > 2) throw costa::engine::error(COSTA_ERR_ARG, "mode must be 0, 1 or 2");
        costa::engine::set_list_builder_mode(mode);
    });
}

int costa_hip_work_export(int dtype, const costa_tile_op_t* ops, int64_t n_ops, int kind, int device,
                          costa_tile_op_t* ordered, int64_t cap_ordered, uint64_t* work,
                          int64_t cap_work, int64_t* meta) {
    auto body = [&] {
        if (!meta || (n_ops > 0 && !ops) || n_ops < 0) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        if (dtype < COSTA_FLOAT || dtype > COSTA_INT32) throw costa::engine::error(COSTA_ERR_ARG, "bad dtype");
        if (kind < 0 || kind > 2) throw costa::engine::error(COSTA_ERR_ARG, "kind must be 0, 1 or 2");
        std::vector<costa_tile_op_t> in(ops, ops + n_ops), o;
        std::vector<uint64_t> w;
        costa::engine::work_split ws;
        const bool on_gpu = costa::engine::work_export(
            costa_dtype_t(dtype), in, costa::engine::list_kind(kind), device, o, w, ws);
        const int64_t m[12] = {ws.n_large, ws.n_medium, ws.n_skew, ws.n_cblock, ws.cblock_lds, ws.cb_map,
                               ws.tiny_first, ws.n_tiny, int64_t(o.size()), int64_t(w.size()), on_gpu,
                               int64_t(ws.tr_shape) | int64_t(ws.sq) << 1 | int64_t(ws.full) << 2 |
                                   int64_t(ws.med_full) << 3 | int64_t(ws.med_sq) << 4 |
                                   int64_t(ws.skew_wide) << 5};
        std::memcpy(meta, m, sizeof(m));
        if (ordered && cap_ordered >= int64_t(o.size()) && !o.empty())
            std::memcpy(ordered, o.data(), o.size() * sizeof(o[0]));
        if (work && cap_work >= int64_t(w.size()) && !w.empty()) std::memcpy(work, w.data(), w.size() * sizeof(w[0]));
    };
    return device >= 0 ? gpu_guarded(body) : guarded(body);  // (the host builder touches no GPU)
}

int costa_hip_set_profiling(int on) {
    costa::engine::set_profiling(on != 0);
    return COSTA_OK;
}

int costa_hip_get_stats(costa_stats_t* out, int reset) {
    return guarded([&] {
        if (!out) throw costa::engine::error(COSTA_ERR_ARG, "null argument");
        costa::engine::resolve_pending();  // timings of asynchronous transforms
        *out = costa::engine::stats();
        if (reset) costa::engine::stats() = costa_stats_t{};
    });
}

int costa_hip_set_host_staging(int mode) {
    return guarded([&] {
        if (mode != 0 && mode != 1) throw costa::engine::error(COSTA_ERR_ARG, "mode must be 0 or 1");
        costa::engine::set_host_staging_mode(mode);
    });
}

int costa_hip_release_caches(void) {
    return gpu_guarded([&] { costa::engine::release_caches(); });
}

}  // extern "C"

// ---------------------------------------------------------------- C++ API
namespace costa {
namespace {
void raise(int rc) {
    if (rc != COSTA_OK) throw hip_error(rc, g_last_error);
}
template <typename T>
engine::scal scal_of(T a, T b) {
    engine::scal s;
    std::memcpy(s.alpha.data(), &a, sizeof(T));
    std::memcpy(s.beta.data(), &b, sizeof(T));
    return s;
}
template <typename T>
void run(std::vector<layout_ref<T>>& from, std::vector<layout_ref<T>>& to, const char* trans,
         const T* alpha, const T* beta, costa_comm_t comm) {
    raise(gpu_guarded([&] {
        if (from.size() != to.size())
            throw engine::error(COSTA_ERR_ARG, "costa::transform: from/to sizes differ");
        if (!comm) throw engine::error(COSTA_ERR_ARG, "costa::transform: null communicator");
        std::vector<engine::elayout> es;
        es.reserve(2 * from.size());
        std::vector<engine::job> jobs(from.size());
        for (size_t i = 0; i < from.size(); ++i) {
            es.push_back(engine::erase(from[i].get()));
            jobs[i].A = &es.back();
            es.push_back(engine::erase(to[i].get()));
            jobs[i].C = &es.back();
            jobs[i].trans = trans ? trans[i] : 'N';
            jobs[i].s = alpha ? scal_of(alpha[i], beta[i]) : scal_of(T{1}, T{0});
        }
        engine::transform(jobs, comm->c);
    }));
}
}  // namespace

template <typename T>
void transform(grid_layout<T>& A, grid_layout<T>& C, costa_comm_t comm) {
    std::vector<layout_ref<T>> f{A}, t{C};
    run<T>(f, t, nullptr, nullptr, nullptr, comm);
}

template <typename T>
void transform(grid_layout<T>& A, grid_layout<T>& C, char trans, T alpha, T beta,
               costa_comm_t comm) {
    std::vector<layout_ref<T>> f{A}, t{C};
    run<T>(f, t, &trans, &alpha, &beta, comm);
}

template <typename T>
void transform(std::vector<layout_ref<T>>& from, std::vector<layout_ref<T>>& to,
               costa_comm_t comm) {
    run<T>(from, to, nullptr, nullptr, nullptr, comm);
}

template <typename T>
void transform(std::vector<layout_ref<T>>& from, std::vector<layout_ref<T>>& to, const char* trans,
               const T* alpha, const T* beta, costa_comm_t comm) {
    run<T>(from, to, trans, alpha, beta, comm);
}

template <typename T>
void transform_triangular(grid_layout<T>& A, grid_layout<T>& C, char trans, char uplo, int k, T alpha,
                          T beta, costa_comm_t comm) {
    raise(gpu_guarded([&] {
        if (!comm) throw engine::error(COSTA_ERR_ARG, "costa::transform_triangular: null communicator");
        const char ul = char(std::toupper(static_cast<unsigned char>(uplo)));
        if (ul != 'U' && ul != 'L')
            throw engine::error(COSTA_ERR_ARG, "costa::transform_triangular: uplo must be 'U' or 'L'");
        engine::elayout a = engine::erase(A), c = engine::erase(C);
        engine::job jb;
        jb.A = &a;
        jb.C = &c;
        jb.trans = trans;
        jb.s = scal_of(alpha, beta);
        jb.uplo = ul;
        jb.k = k;
        engine::transform({jb}, comm->c);
    }));
}
#define COSTA_INSTANTIATE_TRI(T)                                                                  \
    template void transform_triangular<T>(grid_layout<T>&, grid_layout<T>&, char, char, int, T, T, \
                                          costa_comm_t);
COSTA_INSTANTIATE_TRI(float)
COSTA_INSTANTIATE_TRI(double)
COSTA_INSTANTIATE_TRI(std::complex<float>)
COSTA_INSTANTIATE_TRI(std::complex<double>)
COSTA_INSTANTIATE_TRI(int)

// mixed precision: one (A, C) pair, scalars of C's type
template <typename Ta, typename Tc>
void run_mixed(grid_layout<Ta>& A, grid_layout<Tc>& C, char trans, Tc alpha, Tc beta,
               costa_comm_t comm) {
    raise(gpu_guarded([&] {
        if (!comm) throw engine::error(COSTA_ERR_ARG, "costa::transform: null communicator");
        engine::elayout a = engine::erase(A), c = engine::erase(C);
        engine::job jb;
        jb.A = &a;
        jb.C = &c;
        jb.trans = trans;
        jb.s = scal_of(alpha, beta);
        engine::transform({jb}, comm->c);
    }));
}

template <typename Ta, typename Tc>
typename std::enable_if<!std::is_same<Ta, Tc>::value>::type
transform(grid_layout<Ta>& A, grid_layout<Tc>& C, costa_comm_t comm) {
    run_mixed<Ta, Tc>(A, C, 'N', Tc{1}, Tc{0}, comm);
}

template <typename Ta, typename Tc>
typename std::enable_if<!std::is_same<Ta, Tc>::value>::type
transform(grid_layout<Ta>& A, grid_layout<Tc>& C, char trans, Tc alpha, Tc beta, costa_comm_t comm) {
    run_mixed<Ta, Tc>(A, C, trans, alpha, beta, comm);
}

#define COSTA_INSTANTIATE_MIXED(Ta, Tc)                                                         \
    template void transform<Ta, Tc>(grid_layout<Ta>&, grid_layout<Tc>&, costa_comm_t);          \
    template void transform<Ta, Tc>(grid_layout<Ta>&, grid_layout<Tc>&, char, Tc, Tc, costa_comm_t);

COSTA_INSTANTIATE_MIXED(double, float)
COSTA_INSTANTIATE_MIXED(float, double)
COSTA_INSTANTIATE_MIXED(std::complex<double>, std::complex<float>)
COSTA_INSTANTIATE_MIXED(std::complex<float>, std::complex<double>)

#define COSTA_INSTANTIATE_TRANSFORM(T)                                                          \
    template void transform<T>(grid_layout<T>&, grid_layout<T>&, costa_comm_t);                 \
    template void transform<T>(grid_layout<T>&, grid_layout<T>&, char, T, T, costa_comm_t);     \
    template void transform<T>(std::vector<layout_ref<T>>&, std::vector<layout_ref<T>>&,        \
                               costa_comm_t);                                                   \
    template void transform<T>(std::vector<layout_ref<T>>&, std::vector<layout_ref<T>>&,        \
                               const char*, const T*, const T*, costa_comm_t);

COSTA_INSTANTIATE_TRANSFORM(float)
COSTA_INSTANTIATE_TRANSFORM(double)
COSTA_INSTANTIATE_TRANSFORM(std::complex<float>)
COSTA_INSTANTIATE_TRANSFORM(std::complex<double>)
COSTA_INSTANTIATE_TRANSFORM(int)

}  // namespace costa
