/*
 * costa-mi355x — C ABI of the MI355X-native COSTA tile path (libcosta_amd.so).
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * Every entry point returns a status code (COSTA_OK == 0); the message of the last
 * failure on the calling thread is available from costa_hip_last_error().
 * Exceptions never cross this boundary.
 *
 * Which reference interface each entry point replaces (paths under eth-cscs/COSTA):
 *
 *   costa_hip_block_cyclic_layout   costa::block_cyclic_layout<T>   src/costa/layout.hpp:70-86
 *   costa_hip_custom_layout         costa::custom_layout<T>         src/costa/layout.hpp:34-42
 *   costa_hip_transform             costa::transform<T>(A, C, trans, alpha, beta, comm)
 *                                                                  src/costa/grid2grid/transform.hpp:22-27
 *                                   (trans = 'N', alpha = 1, beta = 0 gives the no-scale
 *                                    overload transform.hpp:13-16)
 *   costa_hip_transform_batch       costa::transform<T>(vector<layout_ref>..., trans*, alpha*, beta*, comm)
 *                                   and costa::transformer<T>::transform()
 *                                                                  transform.hpp:38-43, transformer.hpp:8-62
 *   costa_hip_layout_reorder_ranks  grid_layout<T>::reorder_ranks   grid2grid/grid_layout.hpp:32-34
 *   costa_hip_copy_and_transform    costa::memory::copy_and_transform<T>
 *                                                                  src/costa/grid2grid/memory_utils.hpp:339-412
 *   costa_hip_execute_tiles         the pack / local / unpack loops
 *                                   communication_data.cpp:191-217 (copy_to_buffer),
 *                                   :219-244 (copy_from_buffer(idx)), :251-302 (copy_local_blocks)
 *   costa_hip_comm_*                the MPI_Comm argument of transform (one rank per GPU; the data
 *                                   exchange of exchange_async, transform.cpp:46-128, runs on RCCL)
 *   costa_hip_plan_export           utils::prepare_to_send / prepare_to_recv + communication_data
 *                                   ctor (utils.hpp:123-206, communication_data.cpp:103-164):
 *                                   the tile descriptor lists, host-only, for inspection and tests
 */
#ifndef COSTA_HIP_H
#define COSTA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define COSTA_OK 0
#define COSTA_ERR_ARG 1      /* invalid argument / inconsistent layouts */
#define COSTA_ERR_HIP 2      /* a HIP runtime call failed (e.g. no GPU) */
#define COSTA_ERR_NCCL 3     /* an RCCL call failed */
#define COSTA_ERR_INTERNAL 4 /* anything else (allocation failure, bug) */

/* ---- element types (the reference instantiates float, double, complex<float>,
 *      complex<double>: transform.cpp:284-376; int32 is the element type of the
 *      reference's own unit tests, tests/unit/test_utils.cpp) ---- */
typedef enum {
    COSTA_FLOAT = 0,
    COSTA_DOUBLE = 1,
    COSTA_CFLOAT = 2,  /* std::complex<float>, interleaved re/im */
    COSTA_CDOUBLE = 3, /* std::complex<double>, interleaved re/im */
    COSTA_INT32 = 4,
    COSTA_HALF = 5,    /* IEEE binary16, 2 bytes, raw bits ("Half precision" below) */
    COSTA_BFLOAT16 = 6, /* bfloat16, 2 bytes, raw bits */
    COSTA_FP8_E4M3 = 7, /* OCP e4m3fn, 1 byte, raw bits ("FP8" below) */
    COSTA_FP8_E5M2 = 8, /* OCP e5m2, 1 byte, raw bits */
    COSTA_FP4_E2M1 = 9, /* OCP e2m1, 4 bits, two codes per byte ("MXFP4" below; MX entry points only) */
    COSTA_FP6_E2M3 = 10, /* OCP e2m3, 6 bits, four codes per three bytes ("MXFP6" below; MX entry points only) */
    COSTA_FP6_E3M2 = 11  /* OCP e3m2, 6 bits, packed the same way */
} costa_dtype_t;

typedef struct costa_layout_s* costa_layout_t;
typedef struct costa_comm_s* costa_comm_t;

/* identical to costa::block_t (reference layout.hpp:14-19) */
typedef struct {
    void* data; /* first element of the block (host or device memory) */
    int ld;     /* leading dimension of the block */
    int row;    /* global block-row index */
    int col;    /* global block-column index */
} costa_block_t;

/* ---- tile descriptor: one "copy_and_transform" call in normalised form ----
 * The source tile has `nf` elements along its contiguous (fast) dimension and
 * `ns` along the strided one:  src element (f, s) lives at src + (s*lds + f)*sizeof(T).
 *   copy mode      : dst + (s*ldd + f)*sizeof(T)  = g(src(f, s))
 *   transpose mode : dst + (f*ldd + s)*sizeof(T)  = g(src(f, s))
 * g(x) = x (bit copy)                  scale kind COSTA_SCALE_BITCOPY (copy mode only)
 *      = 0                             COSTA_SCALE_ZERO   (alpha == beta == 0)
 *      = alpha*op(x)                   COSTA_SCALE_ALPHA  (beta == 0: C is not read)
 *      = beta*dst + alpha*op(x)        COSTA_SCALE_AXPBY
 * with op = conj when COSTA_TILE_CONJ is set.  Exactly the branches of
 * memory_utils.hpp:20-51 and 101-291.  `src`/`dst` are byte offsets added to the
 * launch's base pointers (absolute addresses when the base is NULL). */
#define COSTA_TILE_TRANSPOSE 0x1u
#define COSTA_TILE_CONJ 0x2u
#define COSTA_TILE_VEC_SRC 0x4u /* src tile columns may be read as 16-byte vectors: 16-byte aligned, or
                                  (4-byte elements, ops of at least one large sub-tile) dword aligned;
                                  the planner sets it for 16-byte alignment, the executor's work
                                  lists add the dword-aligned case */
#define COSTA_TILE_VEC_DST 0x8u /* dst tile rows/columns are 16-byte aligned */
#define COSTA_SCALE_SHIFT 4
#define COSTA_SCALE_MASK 0x30u
#define COSTA_SCALE_BITCOPY 0u
#define COSTA_SCALE_ZERO 1u
#define COSTA_SCALE_ALPHA 2u
#define COSTA_SCALE_AXPBY 3u
#define COSTA_SLOT_SHIFT 16 /* bits 16..31: index of the (alpha, beta) pair */

typedef struct {
    uint64_t src;
    uint64_t dst;
    int32_t nf;
    int32_t ns;
    int32_t lds;
    int32_t ldd;
    uint32_t flags;
    uint32_t order; /* locality hint: the executor may run ops in ascending `order` (ops are
                       independent, so any order gives the same result); the planner sets
                       the tile's rank in column-major order of its target coordinates, so
                       tiles sharing partially used cache lines run together.  0 = none. */
} costa_tile_op_t; /* 40 bytes */

/* ---- edge tile of a triangular (masked) transform: a tile op that writes only the elements on
 * one side of a diagonal.  In the op's own source coordinates (f, s) element (f, s) is kept when
 *   s - f >= diag      (COSTA_TRI_LE clear)
 *   s - f <= diag      (COSTA_TRI_LE set)
 * whatever the orderings and the transpose; kept elements are computed exactly as costa_tile_op_t
 * computes them, every other destination byte is neither read nor written, and source values at
 * dropped positions never influence the result. */
#define COSTA_TRI_LE 0x40u /* flag bit 6 of op.flags: the sense of the comparison */
typedef struct {
    costa_tile_op_t op;
    int32_t diag;
    int32_t pad; /* 0 */
} costa_tri_op_t; /* 48 bytes */

/* ---- tile op of a scaled transform ("scaled transforms" below): a tile op whose source value x
 * is replaced by (x * r[i]) * c[j], (i, j) being the element's target coordinates.  (row0, col0)
 * are the target coordinates of the op's source element (f, s) = (0, 0), counted from the first
 * row and column of C's matrix; with COSTA_SCALED_F_ROWS set the op's fast index f walks target
 * rows and s target columns (i = row0 + f, j = col0 + s), else the other way round (i = row0 + s,
 * j = col0 + f) -- the planner sets it when the source's ordering is column-major != the job
 * transposes.  COSTA_SCALE_BITCOPY of a scaled op means cvt(s_ij(x)), never a byte copy. */
#define COSTA_SCALED_F_ROWS 0x80u /* flag bit 7 of op.flags */
typedef struct {
    costa_tile_op_t op;
    int32_t row0;
    int32_t col0;
} costa_scaled_op_t; /* 48 bytes */

/* ---- library ---- */
const char* costa_hip_last_error(void);
int costa_hip_version(void); /* major*10000 + minor*100 + patch */
int costa_hip_device_count(int* count); /* visible GPUs (COSTA_ERR_HIP without a GPU) */
/* the RCCL library the exchange runs on in this process (ncclGetVersion: major*10000 +
 * minor*100 + patch); which one the loader bound depends on what the process loaded first
 * (torch ships its own librccl under the same soname) */
int costa_hip_rccl_version(int* version);

/* ---- layouts (pointers may be host or device memory; never dereferenced
 *      until a transform runs) ---- */
int costa_hip_block_cyclic_layout(costa_dtype_t dtype, int m, int n, int block_m, int block_n,
                                  int i, int j, int sub_m, int sub_n, int p_m, int p_n,
                                  char rank_grid_ordering, int rsrc, int csrc, void* ptr, int lld,
                                  char data_ordering, int rank, costa_layout_t* out);
int costa_hip_custom_layout(costa_dtype_t dtype, int rowblocks, int colblocks, const int* rowsplit,
                            const int* colsplit, const int* owners, int nlocalblocks,
                            const costa_block_t* localblocks, char ordering, costa_layout_t* out);
void costa_hip_layout_destroy(costa_layout_t layout);
/* rank relabelling: owner(i, j) becomes reordering[owner(i, j)] (replaces any earlier one;
 * n = 0 restores the identity).  Replaces grid_layout<T>::reorder_ranks
 * (src/costa/grid2grid/grid_layout.hpp:32-34, grid2D.hpp:183-187, 219-221).  `reordering` must
 * be a permutation of 0..n-1 (COSTA_ERR_ARG otherwise) with n >= the layout's ranks.  A cell of
 * base owner o then belongs to rank reordering[o], so the process of rank r must hold the local
 * blocks of base rank o with reordering[o] == r (the inverse permutation at r).  The
 * permutations costa::optimal_reordering proposes (<costa/grid2grid/ranks_reordering.hpp>) swap
 * pairs of ranks, i.e. are their own inverse: then rank r holds the blocks of rank
 * reordering[r], as the reference's README puts it (README.md:343-362). */
int costa_hip_layout_reorder_ranks(costa_layout_t layout, const int* reordering, int n);
/* number of local blocks / the i-th block (global intervals, data pointer, ld) */
int costa_hip_layout_num_blocks(costa_layout_t layout);
/* rows (*m) and columns (*n) of the matrix the layout describes (the extent of its splits) */
int costa_hip_layout_shape(costa_layout_t layout, int* m, int* n);
int costa_hip_layout_block(costa_layout_t layout, int i, int* row_start, int* row_end,
                           int* col_start, int* col_end, void** data, int* ld);

/* ---- communicators: one process per GPU ----
 * costa_hip_comm_self: a single-rank communicator on `device` (no RCCL).
 * costa_hip_comm_create: rank `rank` of `nranks`; `id` is the 128-byte RCCL unique id made by
 * costa_hip_comm_unique_id on one rank and broadcast by the caller's control plane (MPI,
 * torch.distributed store, ...).  Collective over all ranks. */
int costa_hip_comm_self(int device, costa_comm_t* out);
int costa_hip_comm_unique_id(unsigned char id[128]);
int costa_hip_comm_create(const unsigned char id[128], int nranks, int rank, int device,
                          costa_comm_t* out);
int costa_hip_comm_rank(costa_comm_t comm);
int costa_hip_comm_size(costa_comm_t comm);
void costa_hip_comm_destroy(costa_comm_t comm);

/* ---- test modes: the exchange path of several ranks on one GPU ----
 * COSTA_LOOPBACK=1 or 2 (environment): a one-rank communicator gets a one-rank RCCL communicator
 * and routes its own tiles (all, or half of them) through PACK -> ncclSend / ncclRecv to itself
 * -> UNPACK.  One rank's geometry, one peer, displacement 0.
 *
 * Rank emulation: the plans and work lists of rank `rank` of `nranks`, without RCCL.
 * costa_hip_comm_emulated makes a communicator that is planned exactly like an RCCL communicator
 * of that rank and size (exchange rounds, pack / unpack lists, plan-cache key).
 * costa_hip_comm_emulate selects what the following transform calls on it launch:
 *   COSTA_EMULATE_PACK    round `round`'s pack lists, into `buffer`, the caller's send package;
 *   COSTA_EMULATE_UNPACK  round `round`'s unpack lists (the triangular and scaled ones included),
 *                         from `buffer`, the caller's receive package;
 *   COSTA_EMULATE_LOCAL   the LOCAL lists (`round` and `buffer` are ignored).
 * `round` is 0 .. costa_hip_exchange_rounds() - 1, or -1 for every round in order.  `buffer` is a
 * device pointer aligned to 256 bytes that holds the plan's send_elems / recv_elems package
 * elements (costa_hip_plan_export*), else COSTA_ERR_ARG.  Each call uploads the scalars, launches
 * the part with the functions every transform uses and synchronises.  The caller is the exchange:
 * between PACK(r) and UNPACK(r) it copies, for every pair of ranks, the element range
 * costa_hip_round_range gives for the pair's count, from the sender's package at the pair's send
 * displacement to the receiver's at its receive displacement (tests/emulated_ranks.py).  Every
 * transform entry point works; COSTA_ERR_ARG for an emulated communicator with no part selected,
 * for host-resident layouts, for the _async forms, and from costa_hip_comm_emulate for a
 * communicator that is not emulated.  Statistics: launches and items are counted per call, the
 * plan's pack_bytes / unpack_bytes with the last round, `transforms` with LOCAL.
 *
 * costa_hip_exchange_rounds: the parts a peer's package of at least 16 MiB is exchanged in
 * (COSTA_EXCHANGE_ROUNDS, default 4).  costa_hip_round_range: the element range [lo, hi) that
 * round `round` of `rounds` moves of a package of `count` elements of `elem_bytes` bytes (one part
 * below the threshold; rounds past the parts are empty at `count`).  Both are host-only.  The
 * threshold has a tuning override, COSTA_ROUND_MIN_BYTES (read only with COSTA_TUNING=1). */
#define COSTA_EMULATE_PACK 1
#define COSTA_EMULATE_UNPACK 2
#define COSTA_EMULATE_LOCAL 3
int costa_hip_comm_emulated(int rank, int nranks, int device, costa_comm_t* out);
int costa_hip_comm_emulate(costa_comm_t comm, int part, int round, void* buffer);
int costa_hip_exchange_rounds(void);
int costa_hip_round_range(int64_t count, int elem_bytes, int rounds, int round, int64_t* lo,
                          int64_t* hi);

/* ---- transforms: sub(C) = beta*sub(C) + alpha*op(sub(A)), op in {'N','T','C'} ----
 * alpha/beta point to ONE element of the layouts' dtype (complex: two reals).
 * Collective over `comm`; blocking (returns after C is complete).
 *
 * Mixed precision (MI355X-native; the reference's transform<T> takes one T): A and C may differ
 * in dtype, COSTA_FLOAT <-> COSTA_DOUBLE or COSTA_CFLOAT <-> COSTA_CDOUBLE, and then
 *   sub(C) = beta*sub(C) + alpha*op(convert(sub(A))),
 * convert being the C++ static_cast from A's element type to C's (round to nearest even,
 * overflow to +-inf, fp32 subnormals kept, widening exact, complex per component).  alpha/beta
 * are ONE element of C's dtype and everything after the conversion runs in C's type with the
 * same-type code: the result equals, bit for bit, the same-type transform of an A converted
 * first.  The conversion runs inside the tile kernels (no temporary); the packages of the
 * exchange hold the narrower of the two types (narrowing pairs convert while packing, widening
 * pairs while unpacking).  Every pair of a batch must share one (A dtype, C dtype); any other
 * unequal pair (COSTA_INT32 with anything, real with complex) is COSTA_ERR_ARG with a message
 * naming both types.  Mixed transforms need device-resident layouts (blocking and _async entry
 * points, any communicator size): on host-resident layouts they return COSTA_ERR_ARG.
 *
 * Half precision (MI355X-native): COSTA_HALF and COSTA_BFLOAT16 are 2-byte element types held as
 * raw bits; offsets, leading dimensions and counts are in elements as for every other type.  Write
 * H for one of the two.  The supported (A, C) pairs are H -> H of the same H, COSTA_FLOAT -> H and
 * H -> COSTA_FLOAT; every other pair with a 2-byte type (COSTA_HALF <-> COSTA_BFLOAT16, H with
 * COSTA_DOUBLE, COSTA_INT32 or a complex type) is COSTA_ERR_ARG with a message naming both types.
 * Whenever A or C is 2-byte, alpha/beta are ONE fp32 each (not an element of C's dtype): the
 * compute type of such a transform is COSTA_FLOAT.  With w() the exact widening to fp32, cvt() the
 * conversion fp32 -> C's type (round to nearest even, overflow to +-inf, subnormals kept) and
 * F(a, c) the COSTA_FLOAT same-type transform of one element (same branches, same operation
 * order, no fma):
 *   H -> H            C = cvt(F(w(A), w(C)))      (scale kind BITCOPY -- copy mode, alpha = 1,
 *                                                  beta = 0 -- is a byte copy)
 *   COSTA_FLOAT -> H  the H -> H transform of cvt(A): A is rounded to C's type first
 *   H -> COSTA_FLOAT  C = F(w(A), C)
 * so all arithmetic is fp32 with ONE rounding at the store.  The packages of the exchange hold H
 * for all three pairs (LOCAL and PACK -> UNPACK give the same bits).  'C' is 'T'.  Bytes of C that
 * no tile writes stay bit-identical.  Device-resident layouts only (COSTA_ERR_ARG with
 * "device-resident" otherwise); blocking, _async, batches and any communicator size work;
 * costa_hip_transform_tri, costa_hip_execute_tiles, costa_hip_execute_tiles_tri and
 * costa_hip_copy_and_transform refuse a 2-byte dtype with COSTA_ERR_ARG.  The C++
 * costa::transform<T> overloads and the ScaLAPACK shims take no half types.
 *
 * FP8 (MI355X-native): COSTA_FP8_E4M3 is OCP e4m3fn (bias 7, no infinities, NaN = 0x7F / 0xFF,
 * largest finite 448) and COSTA_FP8_E5M2 is OCP e5m2 (bias 15, infinities and NaNs as IEEE, largest
 * finite 57344).  Both are 1 byte, held as raw bits; offsets, leading dimensions and counts are in
 * elements as for every other type.  Write Q for one of the two.  The supported (A, C) pairs are
 * Q -> Q of the same Q, COSTA_FLOAT -> Q and Q -> COSTA_FLOAT; every other pair with a 1-byte type
 * (e4m3 <-> e5m2, Q with COSTA_HALF, COSTA_BFLOAT16, COSTA_DOUBLE, COSTA_INT32 or a complex type) is
 * COSTA_ERR_ARG with a message naming both types.  alpha/beta are ONE fp32 each and the compute
 * type is COSTA_FLOAT whenever a side is Q.  With w() the exact widening to fp32 and F(a, c) the
 * COSTA_FLOAT same-type transform of one element (same branches, same operation order, no fma):
 *   Q -> Q            C = cvt(F(w(A), w(C)))      (scale kind BITCOPY -- copy mode, alpha = 1,
 *                                                  beta = 0 -- is a byte copy: NaN payloads survive)
 *   COSTA_FLOAT -> Q  C = cvt(F(A, w(C)))
 *   Q -> COSTA_FLOAT  C = F(w(A), C)
 * cvt(), the conversion fp32 -> Q, is what torch-CPU's x.to(torch.float8_e4m3fn) / .to(torch.
 * float8_e5m2) gives: round to nearest even, subnormals kept, the tie below the smallest subnormal
 * to zero, the sign of zero kept, NaN to NaN; e4m3: any value that rounds above 448, and +-inf,
 * becomes NaN (0x7F with the sign bit; 464 is a tie that rounds to 448, 465 becomes NaN); e5m2: any
 * value that rounds above 57344 becomes +-inf (61440 is a tie that rounds to inf).
 * COSTA_FLOAT -> Q differs from COSTA_FLOAT -> H on purpose: A is NOT rounded before the
 * arithmetic.  The point of this leg is quantisation with alpha = 1 / scale, and rounding a value
 * outside Q's range before scaling it destroys it.
 * Packages of the exchange: Q -> Q and Q -> COSTA_FLOAT carry Q (PACK is a byte copy of 1-byte
 * tiles, UNPACK converts); COSTA_FLOAT -> Q carries COSTA_FLOAT (PACK is an ordinary same-type
 * COSTA_FLOAT list, UNPACK converts): the package type is A's although it is the wider one.  In all
 * three pairs a tile gives the same bits whether it stays local or crosses.
 * As for the half types: 'C' is 'T'.  Bytes of C that no tile writes stay bit-identical.
 * Device-resident layouts only (COSTA_ERR_ARG with "device-resident" otherwise); blocking, _async,
 * batches and any communicator size work, one (A, C) pair per batch; costa_hip_transform_tri,
 * costa_hip_plan_export_tri, costa_hip_execute_tiles, costa_hip_execute_tiles_tri and
 * costa_hip_copy_and_transform refuse a 1-byte dtype with COSTA_ERR_ARG.  The C++
 * costa::transform<T> overloads and the ScaLAPACK shims take no FP8 types. */
int costa_hip_transform(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                        const void* beta, costa_comm_t comm);
/* several layout pairs in one exchange; trans/alpha/beta are arrays of n entries
 * (alpha/beta: n elements of the dtype). */
int costa_hip_transform_batch(int n, const costa_layout_t* A, const costa_layout_t* C,
                              const char* trans, const void* alpha, const void* beta,
                              costa_comm_t comm);

/* ---- triangular / trapezoidal transforms (MI355X-native; ScaLAPACK's p?trmr2d is the copy) ----
 *   C(i, j) = beta*C(i, j) + alpha*op(A)(i, j)   where keep(i, j)
 *   C(i, j) untouched, bit for bit               elsewhere
 *   keep(i, j) = (j - i >= k) for uplo 'U' (numpy triu(k)), (j - i <= k) for uplo 'L' (tril(k)),
 * i, j counted from the first row and column of the matrix C's layout describes (its
 * rows_split / cols_split front; the sub-matrix origin of a block-cyclic layout built over a
 * sub-matrix).  `uplo` is 'U' or 'L' in either case (anything else: COSTA_ERR_ARG), `k` any int: a
 * mask that keeps everything is the ordinary transform, one that keeps nothing is a no-op.  Kept
 * elements equal the ordinary transform's bit for bit; dropped bytes of C are never written, and
 * A's values at dropped positions (NaN, Inf) never reach C.  Tiles wholly outside the mask are
 * neither packed, exchanged nor unpacked.  A and C must share one dtype (COSTA_ERR_ARG otherwise);
 * host-resident layouts take the mirror staging, with C's ranges uploaded first.
 *
 * In-place fill of the other triangle: A and C may be layouts over the SAME device buffer of a
 * square matrix when trans is 'T' or 'C' and the mask is strict (uplo 'L' with k <= -1, or 'U'
 * with k >= 1): the elements read for kept positions and the elements written are then disjoint,
 * and values read at dropped positions are discarded.  Device-resident layouts, one rank (also
 * through the loopback test mode). */
int costa_hip_transform_tri(costa_layout_t A, costa_layout_t C, char trans, char uplo, int k,
                            const void* alpha, const void* beta, costa_comm_t comm);
int costa_hip_transform_tri_async(costa_layout_t A, costa_layout_t C, char trans, char uplo, int k,
                                  const void* alpha, const void* beta, costa_comm_t comm,
                                  void* stream);

/* ---- scaled transforms (MI355X-native): row / column scale vectors fused into the tile kernels ----
 * With m x n the matrix C's layout describes and i, j counted from its first row and column (the
 * origin costa_hip_transform_tri documents):
 *   C(i, j) = beta*C(i, j) + alpha * s_ij(op(A)(i, j)),      s_ij(x) = (x * r[i]) * c[j]
 * `row_scale` (r, m elements) and `col_scale` (c, n elements) are DEVICE arrays of the compute type
 * (float; double for the COSTA_DOUBLE pair), replicated on every rank.  Either may be NULL: its
 * multiplication is then skipped (not replaced by a multiplication by 1).  Both NULL is
 * COSTA_ERR_ARG ("use costa_hip_transform"); a host pointer for a vector is COSTA_ERR_ARG with
 * "device-resident" in the message.  The vectors are read during the call; for the _async form
 * they must stay valid until the stream has passed the call.  Their addresses and values are not
 * part of the plan: one cached plan serves every vector, present or absent.
 *
 * Bit-level definition: the ordinary transform of the same (A, C) pair whose arithmetic reads
 * s_ij(x) wherever it would read x.  x is the source value as the pair delivers it to its
 * arithmetic: w(A) for 2-byte (H) and 1-byte (Q) sources, w(cvt_H(A)) for COSTA_FLOAT -> H (the
 * package keeps holding H), the unrounded A for COSTA_FLOAT -> Q and COSTA_FLOAT -> COSTA_FLOAT.
 * The two products are two separately rounded multiplications in the compute type, r first, no
 * fma; then the unchanged scale branches (ZERO, ALPHA, AXPBY) and one cvt() at the store.  Scale
 * kind BITCOPY (copy mode, alpha = 1, beta = 0) means cvt(s_ij(x)) here, never a byte copy.  'C'
 * is 'T' (real types only).  Bytes of C that no tile writes keep their bits.
 *
 * Accepted (A, C) pairs -- every pair costa_hip_transform accepts whose compute type is real
 * COSTA_FLOAT, plus COSTA_DOUBLE -> COSTA_DOUBLE: COSTA_FLOAT -> COSTA_FLOAT, the six half pairs
 * (H -> H, COSTA_FLOAT -> H, H -> COSTA_FLOAT), the six FP8 pairs, COSTA_DOUBLE -> COSTA_DOUBLE.
 * Everything else (complex, COSTA_INT32, COSTA_FLOAT <-> COSTA_DOUBLE, and the pairs
 * costa_hip_transform refuses) is COSTA_ERR_ARG with a message naming both types.
 * Device-resident layouts only (COSTA_ERR_ARG with "device-resident" otherwise); blocking and
 * _async; any communicator size (the exchange is the ordinary plan's: only LOCAL and UNPACK ops
 * scale).  No batches, no triangular mask, no host staging.
 *
 * In place: A and C may be the SAME layout over the same device buffer when trans is 'N':
 * A <- diag(r) * A * diag(c) (p?laqge).  Every op is then a LOCAL copy-mode op whose source and
 * destination coincide, and every lane of the kernel stores exactly the elements it loaded (the
 * kernel's data pointers carry no __restrict__).  Device-resident layouts, one rank. */
int costa_hip_transform_scaled(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                               const void* beta, const void* row_scale, const void* col_scale,
                               costa_comm_t comm);
int costa_hip_transform_scaled_async(costa_layout_t A, costa_layout_t C, char trans,
                                     const void* alpha, const void* beta, const void* row_scale,
                                     const void* col_scale, costa_comm_t comm, void* stream);

/* ---- amax outputs (MI355X-native): row / column abs-max fused into the scaled kernels ----
 * The statistic per-channel quantisation needs (row_scale = 448 / amax), taken from a distributed
 * matrix without leaving the device: only the layout knows which global row and column an element
 * of a padded local buffer belongs to.
 *
 * Definition.  Tc is the real compute type (float; double for the COSTA_DOUBLE pair) and U the
 * unsigned integer of its width.  absbits(x) is the bits of x with the sign bit cleared: no
 * arithmetic, so denormals are not flushed and -0 becomes +0.  An amax vector is a DEVICE array of
 * Tc, and an update over a set of elements x is
 *   v[k] <- the value whose bits are  umax(bits(v[k]), absbits(x)),   compared as U.
 * For non-NaN values that is the exact maximum of |x|.  A NaN outranks everything, so the entry
 * becomes a NaN (which payload is not specified).  umax is associative and commutative: the result
 * does not depend on the order the kernels run in.  The update ACCUMULATES: the caller initialises
 * the vector, normally to zeros, and several calls may update the same vector.  On entry every
 * entry must have a clear sign bit (a non-negative value, +0, +inf or a NaN without the sign bit):
 * an entry with the sign bit set compares above every |x| and would stay.  An amax vector must not
 * overlap a scale vector or a layout's data.
 *
 * Fused form, costa_hip_transform_amax: computes exactly what costa_hip_transform_scaled computes
 * with the same arguments, except that BOTH scale vectors may be NULL here: the result is then the
 * scaled definition with both products skipped -- it still runs through scaled_kernel, and scale
 * kind BITCOPY still means cvt(x).  In addition, for every element (i, j) of C's matrix that this
 * rank writes (its LOCAL and UNPACK ops), row_amax[i] (m elements) and col_amax[j] (n elements) are
 * updated with x, the value the scaled section defines as "the source value as the pair delivers it
 * to its arithmetic": w(A) for H / Q sources, w(cvt_H(A)) for COSTA_FLOAT -> H (the package holds
 * H, an UNPACK op has nothing else), the unrounded A otherwise -- before the scale products and
 * before alpha / beta.  Either amax vector may be NULL; both NULL is COSTA_ERR_ARG ("use
 * costa_hip_transform_scaled or costa_hip_transform").  A host pointer for an amax vector is
 * COSTA_ERR_ARG with "device-resident" in the message.  Accepted pairs, refusals and their messages
 * are those of scaled transforms; device-resident layouts only, any communicator size, no batches,
 * no triangular mask.  The plan is the scaled plan: the amax addresses are not part of it, and one
 * cached plan serves scaled and amax calls alike.  Calls without an amax vector launch exactly the
 * kernels they launched before this section existed.
 * Several ranks: each rank's vectors hold the maxima over that rank's OWN part of C; the caller
 * max-reduces them across ranks (for non-NaN data an ordinary floating-point max all-reduce).
 * In place (A and C the same layout, 'N') works as for scaled transforms; the amax is that of the
 * matrix BEFORE scaling (the kernel holds x in registers before it stores).
 * For the _async form the vectors must stay valid until the stream has passed the call.
 *
 * Reduce-only form, costa_hip_layout_amax: updates row_amax / col_amax with w(a) for every element
 * a of the layout's local blocks; the vectors are indexed by the rows and columns of A's matrix,
 * from the origin of costa_hip_layout_shape.  The widening is exact and no pair is involved.
 * Nothing is written except the vectors; there is no exchange and no plan: the communicator
 * supplies the device and the call ordering (calls run in order with the transforms of the
 * process).  Element types COSTA_FLOAT, COSTA_DOUBLE (vectors of double), COSTA_HALF,
 * COSTA_BFLOAT16, COSTA_FP8_E4M3, COSTA_FP8_E5M2; complex types and COSTA_INT32 are COSTA_ERR_ARG
 * naming the type.  Device-resident layouts only; either vector may be NULL, not both.
 *
 * Two recipes.  Delayed scaling: costa_hip_transform_amax with the previous
 * step's scales and this step's amax outputs, one pass.  Current scaling: costa_hip_layout_amax,
 * the scales computed from the vectors on the device, then costa_hip_transform_scaled. */
int costa_hip_transform_amax(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                             const void* beta, const void* row_scale, const void* col_scale,
                             void* row_amax, void* col_amax, costa_comm_t comm);
int costa_hip_transform_amax_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                   const void* beta, const void* row_scale, const void* col_scale,
                                   void* row_amax, void* col_amax, costa_comm_t comm, void* stream);
int costa_hip_layout_amax(costa_layout_t A, void* row_amax, void* col_amax, costa_comm_t comm);
int costa_hip_layout_amax_async(costa_layout_t A, void* row_amax, void* col_amax, costa_comm_t comm,
                                void* stream);

/* ---- MX block-scaled transforms (MI355X-native): E8M0 scales per 32 elements, fused ----
 * FP8 data with one power-of-two scale byte (E8M0) per 32 consecutive elements along one axis (OCP
 * Microscaling v1.0, MXFP8), produced or consumed by the redistribution itself in one pass.
 *
 * Scale tensor.  A DEVICE array of bytes described by costa_mx_scales_t.  With axis COSTA_MX_ROWS a
 * block is 32 consecutive ROWS of one column: block b of line l covers rows 32b .. 32b+31 of column
 * l.  With COSTA_MX_COLS a block is 32 consecutive COLUMNS of one row (l is the row).  The byte of
 * (b, l) is data[b*block_stride + l*line_stride] (block-major or line-major storage is the caller's
 * choice).  Coordinates count from the first row and column of the layout's matrix, as for the scale
 * vectors above: `a_scales` is indexed by A's matrix as stored (before op), `c_scales` by C's.  The
 * last block of a line may be partial and reduces over the elements that exist.  Both strides must
 * be positive and no two (b, l) of the matrix may share a byte (COSTA_ERR_ARG otherwise).
 *
 * Byte encoding.  pow2(E) is the fp32 with bits E << 23 for 1 <= E <= 254; pow2(0) = 0x00400000
 * (2^-127, a subnormal, not flushed); pow2(255) = 0x7FC00000 (NaN).
 *
 * Arithmetic (fp32, no contraction).  For each written element:
 *   1. x = w(a); with a_scales  x = x * pow2(SA[block of a])  (one rounded product)
 *   2. v = g(x, w(c_old)): the ordinary ZERO / ALPHA / AXPBY branches (BITCOPY: v = x)
 *   3. without c_scales (C is COSTA_FLOAT): store v
 *   4. with c_scales (C is FP8, beta must be 0), per block of C: amax = the unsigned maximum of the
 *      bit patterns of |v| over the block, e = amax >> 23.  e == 255 (an inf or NaN in the block):
 *      E = 255 and every element of the block is stored as a NaN of the type.  Otherwise
 *      E = clamp(e - emax, 0, 254), emax = 8 (e4m3) / 15 (e5m2): the OCP floor rule.  With rounding
 *      COSTA_MX_CEIL E is one higher (at most 254) when amax * pow2(254 - E) > fmax (448 / 57344);
 *      then no element saturates.  q = cvt(clamp(v * pow2(254 - E), -fmax, +fmax)) with the ordinary
 *      round-to-nearest-even cvt; SC[block] = E.  An all-zero block gives E = 0 and zeros.
 *
 * Accepted calls (everything else is COSTA_ERR_ARG naming what was wrong, C and the scale tensors
 * untouched):
 *   quantise    COSTA_FLOAT -> FP8      a_scales NULL, c_scales required, beta = 0
 *   dequantise  FP8 -> COSTA_FLOAT      a_scales required, c_scales NULL, alpha / beta free
 *   requantise  FP8 -> the same FP8     both required, beta = 0 (e.g. 'T' with the other axis)
 * A descriptor is "absent" when its pointer or its `data` is NULL.
 *
 * Tile boundaries.  A block of C must not be split by a tile boundary: along c_scales.axis every
 * LOCAL and UNPACK op of the plan must start at a multiple of 32 of C's coordinates and span a
 * multiple of 32 or end at the matrix edge, i.e. the block sizes and split points of both layouts
 * (A's seen through op) are multiples of 32 along that axis.  Checked before anything is written:
 * COSTA_ERR_ARG with "MX block" in the message.  a_scales has no such restriction.
 *
 * Several ranks.  The exchange is the ordinary plan's (COSTA_FLOAT -> Q sends fp32, Q -> .. sends Q
 * bytes); only LOCAL and UNPACK ops touch scale tensors.  A rank writes only the c_scales bytes of
 * the blocks it owns in C and leaves every other byte alone: zero-initialised tensors merge across
 * ranks with a byte-wise all-reduce MAX.  A rank needs the a_scales bytes of every block it reads,
 * those of tiles it receives included: the library moves no scales between ranks, so replicate
 * a_scales.
 *
 * Device-resident layouts and scale tensors only (a host pointer is COSTA_ERR_ARG with
 * "device-resident"); blocking or _async; any communicator size.  No batches, no triangular mask,
 * no host staging, no in-place calls.  The plan is the scaled plan of the pair (the tensors and the
 * rounding mode are arguments of the call): one cached plan serves scaled, amax and MX calls. */
#define COSTA_MX_ROWS 0
#define COSTA_MX_COLS 1
#define COSTA_MX_FLOOR 0
#define COSTA_MX_CEIL 1
typedef struct {
    void* data;           /* device array of E8M0 bytes */
    int axis;             /* COSTA_MX_ROWS / COSTA_MX_COLS */
    int64_t block_stride; /* bytes between consecutive blocks of one line */
    int64_t line_stride;  /* bytes between the same block of consecutive lines */
} costa_mx_scales_t; /* 32 bytes */
int costa_hip_transform_mx(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                           const void* beta, const costa_mx_scales_t* a_scales,
                           const costa_mx_scales_t* c_scales, int rounding, costa_comm_t comm);
int costa_hip_transform_mx_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                 const void* beta, const costa_mx_scales_t* a_scales,
                                 const costa_mx_scales_t* c_scales, int rounding, costa_comm_t comm,
                                 void* stream);
/* scaled ops (costa_scaled_op_t, as for costa_hip_execute_tiles_scaled) of one accepted MX pair in
 * ONE launch of mx_kernel; fp32 scalars.  m x n is C's matrix (the target coordinates of the ops);
 * with a_transposed != 0 A's matrix is n x m and target (i, j) is A's (j, i), so a_scales is indexed
 * accordingly.  The tile-boundary rule and beta = 0 with c_scales are checked on the ops. */
int costa_hip_execute_tiles_mx(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                               const costa_scaled_op_t* ops, int64_t n_ops, const void* src_base,
                               void* dst_base, const void* scalars, int n_slots,
                               const costa_mx_scales_t* a_scales, const costa_mx_scales_t* c_scales,
                               int rounding, int64_t m, int64_t n, int a_transposed, int device);
/* sub-tiles run by mx_kernel since the last reset; kept beside costa_stats_t, whose layout does not
 * change.  costa_hip_scaled_items / costa_hip_amax_items do not count them. */
int costa_hip_mx_items(int64_t* items, int reset);
/* the tile-boundary rule alone, on caller-given ops (host only, no GPU): COSTA_OK or COSTA_ERR_ARG */
int costa_hip_mx_check_ops(const costa_scaled_op_t* ops, int64_t n_ops, int axis, int64_t m, int64_t n);
/* the stride / aliasing rule of a descriptor for a rows x cols matrix (host only, `data` unused) */
int costa_hip_mx_check_scales(const costa_mx_scales_t* s, int64_t rows, int64_t cols);

/* ---- MXFP4 (MI355X-native): packed e2m1 layouts in the MX block-scaled transforms ----
 * Element type.  COSTA_FP4_E2M1 is OCP e2m1.  A code is 4 bits: bit 3 the sign, bits 2..1 the
 * exponent (bias 1), bit 0 the mantissa; the magnitudes of codes 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6.
 * No infinity, no NaN.
 *
 * Packing.  Two codes share a byte along the layout's stored-contiguous dimension: rows for
 * column-major 'C' storage, columns for 'R'.  Element indices count from the first element of the
 * local block's buffer; the element with the even index sits in bits 3..0, the next one in bits 7..4
 * (the order of torch's float4_e2m1fn_x2 helpers, hi << 4 | lo).
 *
 * Layouts.  Every count of the layout calls stays in ELEMENTS (m, n, block sizes, i / j, sub_m /
 * sub_n, lld / ld, split points); the data pointer addresses bytes and the byte pitch is ld / 2.
 *
 * w4(code) is the exact fp32 value of a code (w4(0x8) = -0.0).  cvt4(t) converts a finite fp32 t
 * with |t| <= 6: round to the nearest representable magnitude, ties to the code whose mantissa bit
 * is 0 (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the sign bit of t is
 * always kept (-0.0 and -0.2 give 0x8).  cvt4(NaN) = 0x0, which occurs only in a block whose scale
 * byte is 255.
 *
 * Block rule.  The MXFP8 rule above with emax = 2 and fmax = 6.0 (bits 0x40C00000): per block of 32
 * elements of C along c_scales.axis, amax = the unsigned maximum of the bits of |v|, e = amax >> 23;
 * e == 255 gives E = 255, else E = max(e - 2, 0); with COSTA_MX_CEIL E is one higher (at most 254)
 * where amax * pow2(254 - E) > 6.0.  q = cvt4(clamp(v * pow2(254 - E), -6, 6)), SC[block] = E; a block
 * with E = 255 stores code 0x0 everywhere.  Under the floor rule a block's maximum lands in [4, 8),
 * so values above 6 saturate: the clamp is load-bearing, as for e4m3.
 *
 * Dequantise.  x = w4(a) * pow2(SA[block]) is one rounded fp32 product; the ordinary alpha / beta
 * branches follow in fp32 with contraction off (beta is free: C is fp32).
 *
 * Accepted calls (costa_hip_transform_mx, _async, costa_hip_execute_tiles_mx; the descriptor,
 * rounding, stride, device-residency and "MX block" checks apply unchanged):
 *   quantise    COSTA_FLOAT -> COSTA_FP4_E2M1     c_scales, beta = 0
 *   dequantise  COSTA_FP4_E2M1 -> COSTA_FLOAT     a_scales
 *   requantise  COSTA_FP4_E2M1 -> COSTA_FP4_E2M1  both, beta = 0
 * COSTA_FP4_E2M1 with any other type is "no MX transform".  Every other entry point refuses an FP4
 * layout or dtype with COSTA_ERR_ARG naming FP4_E2M1, except costa_hip_plan_export_scaled, which
 * plans the three pairs (host only).  In a plan of an FP4 pair every count of an op is in elements
 * and src / dst are byte addresses; when A holds FP4 the package is packed too: its PACK ops are
 * 1-byte copy ops (nf / 2 x ns, pitch lds / 2) and the send / receive counts and displacements count
 * BYTES, so that no round boundary falls inside a byte.
 *
 * Evenness rule ("FP4 pair").  No tile may split a byte.  At layout creation of an FP4 layout: ld
 * is even, and along the packed dimension the matrix extent, the layout's own split points and (for
 * block-cyclic layouts) the sub-matrix offset and every local block offset are even.  At plan time,
 * for every op of the pair on each FP4 side: the op's element offset from its block pointer and its
 * extent along that side's stored-contiguous dimension are even -- through op, the OTHER layout's
 * split points count too.  costa_hip_execute_tiles_mx applies the per-op half (even extent and even
 * leading dimension on each FP4 side) to caller-given ops.  A violation is COSTA_ERR_ARG with "FP4
 * pair" and the offending interval in the message, before anything is written.
 *
 * Not covered: NVFP4 (16-element blocks, e4m3 scales), bf16 / fp16 sides, host-resident FP4
 * layouts, batches, masks, in-place calls, odd extents (a half-filled last byte), swizzled scales. */

/* ---- MXFP6 (MI355X-native): packed e2m3 / e3m2 layouts in the MX block-scaled transforms ----
 * Element types.  COSTA_FP6_E2M3 = 10 and COSTA_FP6_E3M2 = 11 (OCP Microscaling v1.0 FP6).  A code is
 * 6 bits, bit 5 the sign.  Neither type has an infinity or a NaN.
 *          exponent bits (bias)  mantissa bits  magnitudes (mantissa m, exponent e)              largest             emax
 *   e2m3   4..3 (1)              2..0           e = 0: m / 8, else (1 + m / 8) * 2^(e - 1):      7.5 (0x40F00000)    2
 *                                               0, 0.125 .. 0.875, 1 .. 7.5
 *   e3m2   4..2 (3)              1..0           e = 0: m / 16, else (1 + m / 4) * 2^(e - 3):     28 (0x41E00000)     4
 *                                               0, 0.0625, 0.125, 0.1875, 0.25 .. 28
 *
 * Packing.  Four codes share three bytes along the layout's stored-contiguous dimension (rows for
 * 'C', columns for 'R').  Element indices count from the first element of the local block's buffer.
 * Group g holds elements 4g .. 4g + 3 in bytes 3g .. 3g + 2: with w = c0 | c1 << 6 | c2 << 12 |
 * c3 << 18 the bytes are w & 0xFF, (w >> 8) & 0xFF, w >> 16 -- the lowest bits hold the first
 * element, which continues the FP4 rule.
 *
 * Layouts.  Every count of the layout calls stays in ELEMENTS (m, n, block sizes, i / j, sub_m /
 * sub_n, lld / ld, split points).  Pointers address bytes and the byte pitch is 3 * ld / 4.  A block
 * pointer may sit at any byte address: there is no alignment requirement.
 *
 * Codec.  w6(code) is the exact fp32 value; the code with only the sign bit set is -0.0.  cvt6(t),
 * for finite |t| <= fmax, rounds to the nearest representable magnitude; ties go to the code whose
 * mantissa is even (round-to-nearest-even on the dropped bits, subnormals included).  The sign bit of
 * t is always kept: -0.0 and -0.01 give 0x20.  cvt6(NaN) = 0x00, which occurs only in a block whose
 * scale byte is 255.
 *
 * Block rule.  The MXFP8 rule with the type's emax and fmax: per block of 32 elements of C along
 * c_scales.axis, amax = the unsigned maximum of the bits of |v|, e = amax >> 23; e == 255 gives
 * E = 255 and the block stores code 0x00 everywhere, else E = max(e - emax, 0); with COSTA_MX_CEIL E
 * is one higher (at most 254) where amax * pow2(254 - E) > fmax.  q = cvt6(clamp(v * pow2(254 - E),
 * -fmax, fmax)), SC[block] = E.  Under the floor rule a block's maximum lands in [4, 8) for e2m3 and
 * [16, 32) for e3m2; values above 7.5 / 28 saturate, so the clamp is load-bearing.
 *
 * Dequantise.  x = w6(a) * pow2(SA[block]) is one rounded fp32 product; the ordinary alpha / beta
 * branches follow in fp32 with contraction off.
 *
 * Accepted calls (costa_hip_transform_mx, _async, costa_hip_execute_tiles_mx; the descriptor,
 * rounding, stride, device-residency, in-place and "MX block" checks apply unchanged), for each FP6
 * type P:
 *   quantise    COSTA_FLOAT -> P   c_scales, beta = 0
 *   dequantise  P -> COSTA_FLOAT   a_scales
 *   requantise  P -> P             both, beta = 0
 * P with any other type is COSTA_ERR_ARG "no MX transform", naming both types: the other FP6 type,
 * FP4, FP8, half, double, int32 and complex.  Every other entry point refuses an FP6 layout or dtype
 * with COSTA_ERR_ARG naming the type, except costa_hip_plan_export_scaled, which plans the six pairs
 * (host only).
 *
 * Quad rule ("FP6 quad").  No tile may split a 3-byte group.  At creation of an FP6 layout: ld is a
 * multiple of 4, and along the packed dimension the matrix extent, the layout's own split points and
 * (block-cyclic) the sub-matrix offset, the sub-matrix extent and every local block offset are
 * multiples of 4.  At plan time, for every op on each FP6 side: the op's element offset from its
 * block pointer and its extent along that side's stored-contiguous dimension are multiples of 4 --
 * through op, the OTHER layout's split points count too.  costa_hip_execute_tiles_mx applies the
 * per-op half (extent and leading dimension) to caller-given ops.  A violation is COSTA_ERR_ARG with
 * "FP6 quad", the type's name and the offending interval, raised before anything is written.
 *
 * Package.  When A holds FP6 the package is packed: its PACK ops are 1-byte copy ops (3 nf / 4 x ns,
 * pitch 3 lds / 4) and the send / receive counts and displacements count BYTES.  A round boundary may
 * fall inside a group but never inside an op's bytes: ops are assigned to rounds whole.
 * COSTA_FLOAT -> P sends fp32, as for FP8 / FP4.
 *
 * Not covered: NVFP4, bf16 / fp16 sides, host-resident packed layouts, batches, masks, in-place
 * calls, extents off the grid of 4 (2 for FP4), swizzled scales, FP6 <-> FP4 / FP8 requantise. */

/* ---- Stochastic rounding in the MX transforms (MI355X-native): seeded, position-keyed ----
 * The quantise (COSTA_FLOAT -> Q) and requantise (Q -> the same Q) legs of the MX transforms with
 * stochastic rounding (SR) in place of round-to-nearest-even, for the five Q types: FP8 e4m3 / e5m2,
 * FP4 e2m1, FP6 e2m3 / e3m2.  The rounding decision of an element depends on three things only: the
 * call's 64-bit seed, the element's row i and column j in C's matrix (zero-based, the coordinates
 * c_scales is indexed by) and its value.  The same call therefore gives the same bytes whatever the
 * layouts, tile cuts, rank count and kernel mode, and on every run.
 *
 * Arithmetic.  Steps 1 - 4 of "MX block-scaled transforms" (and of MXFP4 / MXFP6) stay as they are up
 * to and including the block's E (floor or ceil rule) and t = clamp(v * pow2(254 - E), -fmax, +fmax):
 * the scale bytes are those of the round-to-nearest call, and a block with E = 255 is stored as there
 * (NaN codes for FP8, code 0 for FP4 / FP6).  Only cvt changes.
 *
 * Random bits (uint32 arithmetic, wrapping):
 *   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *   k0 = fmix32(uint32(seed)       ^ 0x9E3779B9)
 *   k1 = fmix32(uint32(seed >> 32) ^ 0x85EBCA6B)
 *   U(seed, i, j) = fmix32((fmix32(uint32(i) ^ k0) + uint32(j)) ^ k1) >> 8          24 bits
 * Known answers: fmix32(1) = 0x514E28B7; the keys of seed 0 are (0x92CA2F0E, 0xCB72770F), those of
 * seed 0x0123456789ABCDEF (0x089887A8, 0x66EA390A); U at (0,0), (1,2), (202,157), (70000,3) is
 * 0x40042D, 0x0C4B6B, 0x09E145, 0x0982E5 for seed 0x0123456789ABCDEF and 0x2D3D8A, 0xECE447, 0x5F71F2,
 * 0x40208F for seed 0.
 *
 * Conversion.  Let a = |t| and m_0 = 0 < m_1 < .. < m_K = fmax the finite magnitudes of Q in code
 * order; lo = m_k is the largest magnitude <= a.  If a == lo the magnitude code is k for every U.
 * Otherwise hi = m_(k+1), T = floor((a - lo) / (hi - lo) * 2^24), and the code is k + 1 when
 * T + U >= 2^24, else k.  The sign bit of t is always kept (-0 and negatives that round to zero
 * included).  So P(up) = T / 2^24 exactly.  For a result in Q's normal range T is the dropped mantissa
 * bits of a shifted to 24 bits: the top 23 - MB bits of U are added below the kept mantissa of a's
 * fp32 pattern and the sum is truncated (a carry moves into the exponent).  Below Q's smallest normal
 * it is the same rule on a in units of the subnormal step with 24 fraction bits, truncated.  After
 * the clamp a <= fmax, so k + 1 never passes fmax (e4m3 never produces 0x7F in a finite block).
 *
 * Calls.  The _sr forms take every argument and every check of their plain forms, with the same
 * messages, and `seed`; `rounding` stays the floor / ceil rule of the scales.  One more check: a
 * dequantise (C is COSTA_FLOAT, no c_scales) is COSTA_ERR_ARG with "stochastic rounding" in the
 * message, C and the tensors untouched.  The seed is an argument of the call, not of the plan: the
 * pair's cached scaled plan serves SR and plain calls of every seed.  Several ranks: unchanged
 * (COSTA_FLOAT -> Q quantises in UNPACK, Q -> .. sends Q bytes); since U is keyed on C's global
 * coordinates every rank computes the bytes a single rank would.  costa_hip_mx_items counts the
 * sub-tiles of SR launches like the others.  Use a fresh seed per call and per tensor.
 *
 * Not covered: SR in costa_hip_transform_block_scaled, in the plain and scaled COSTA_FLOAT -> FP8 /
 * half transforms, the gfx950 stochastic-rounding conversion instructions (their bit selection is
 * not this definition), bf16 sides. */
int costa_hip_transform_mx_sr(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                              const void* beta, const costa_mx_scales_t* a_scales,
                              const costa_mx_scales_t* c_scales, int rounding, uint64_t seed,
                              costa_comm_t comm);
int costa_hip_transform_mx_sr_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                    const void* beta, const costa_mx_scales_t* a_scales,
                                    const costa_mx_scales_t* c_scales, int rounding, uint64_t seed,
                                    costa_comm_t comm, void* stream);
int costa_hip_execute_tiles_mx_sr(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                  const costa_scaled_op_t* ops, int64_t n_ops, const void* src_base,
                                  void* dst_base, const void* scalars, int n_slots,
                                  const costa_mx_scales_t* a_scales, const costa_mx_scales_t* c_scales,
                                  int rounding, int64_t m, int64_t n, int a_transposed, uint64_t seed,
                                  int device);
/* U(seed, i, j) above (host only, no GPU) */
int costa_hip_sr_bits(uint64_t seed, int64_t i, int64_t j, uint32_t* u24);

/* ---- Dual-output MX quantise (MI355X-native): C and its transpose from one pass over A ----
 * The two quantised copies an MX GEMM training step consumes -- op(A) with its blocks along one
 * reduction dimension and op(A)^T with its blocks cut anew along the other -- from ONE read of the
 * fp32 source: one launch per phase, the fp32 package exchanged once.
 *
 * Arguments.  A is COSTA_FLOAT.  C and Ct hold the same Q, one of COSTA_FP8_E4M3, COSTA_FP8_E5M2,
 * COSTA_FP4_E2M1, COSTA_FP6_E2M3, COSTA_FP6_E3M2.  With op(A) an m x n matrix C describes an m x n
 * matrix and Ct an n x m one.  alpha is fp32; there is no beta (both outputs are quantised).
 * `rounding` is the floor / ceil rule, shared by both outputs.  sr_seed == NULL rounds to nearest;
 * otherwise both outputs are those of the _sr calls with *sr_seed, each element's random bits keyed
 * on its row and column in its OWN output's matrix: (i, j) in C, (j, i) in Ct.
 *
 * Result.  The bytes of C and c_scales are those of costa_hip_transform_mx(A, C, trans, alpha,
 * beta = 0, NULL, c_scales, rounding, comm); the bytes of Ct and ct_scales those of the same call on
 * (A, Ct) with the opposite trans ('T' where trans is 'N', 'N' where it is 'T' or 'C').
 *
 * Scale tensors.  c_scales is indexed by C's matrix and ct_scales by Ct's; each has its own axis and
 * strides and all four axis combinations are valid.  The two tensors must not overlap (not checked).
 *
 * Twin rule ("dual layouts").  The plan is the scaled plan of (A, C, trans).  For an op of its LOCAL
 * and UNPACK lists that covers rows [r0, r1) x columns [c0, c1) of C, rows [c0, c1) x columns
 * [r0, r1) of Ct must lie inside one block of Ct that is local to this rank (after any rank
 * relabelling).  Transposed split points with transposed owners always satisfy it, coarser blocks
 * of Ct too.  A violation is COSTA_ERR_ARG with "dual layouts" and the offending rectangle, raised
 * before anything is written.  Since the ops of all ranks tile C exactly once, every element of Ct is
 * then written exactly once.
 *
 * Block rule.  "MX block" holds for each output along its own axis: on C's ops as for
 * costa_hip_transform_mx, and on the transposed ops for Ct; the message says which output failed.
 * The "FP4 pair" / "FP6 quad" rules hold on Ct's side for the transposed ops.
 *
 * Other checks (COSTA_ERR_ARG naming what was wrong; C, Ct and both tensors untouched): A not
 * COSTA_FLOAT, or C and Ct of different types or not an MX type ("no dual MX transform"); Ct's shape
 * not n x m ("dual layouts"); a missing descriptor ("c_scales is required" / "ct_scales is
 * required"); the stride / aliasing rule per tensor against its own matrix; an unknown rounding value;
 * Ct the same layout object as A or C; a host-resident layout or tensor ("device-resident").
 *
 * Several ranks.  The exchange is that of (A, C, trans): fp32 packages, sent once.  Only LOCAL and
 * UNPACK write; a rank writes the scale bytes of the blocks it owns in C and in Ct and no other byte.
 * Emulated communicators and _async work as for costa_hip_transform_mx.  The cached plan is keyed on
 * Ct's layout content too; a plain costa_hip_transform_mx(A, C) keeps its own plan.
 *
 * Not covered: Q or half sources, different Q types for C and Ct, beta, batches, masks, host staging,
 * costa_hip_transform_block_scaled. */
int costa_hip_transform_mx_dual(costa_layout_t A, costa_layout_t C, costa_layout_t Ct, char trans,
                                const void* alpha, const costa_mx_scales_t* c_scales,
                                const costa_mx_scales_t* ct_scales, int rounding, const uint64_t* sr_seed,
                                costa_comm_t comm);
int costa_hip_transform_mx_dual_async(costa_layout_t A, costa_layout_t C, costa_layout_t Ct, char trans,
                                      const void* alpha, const costa_mx_scales_t* c_scales,
                                      const costa_mx_scales_t* ct_scales, int rounding,
                                      const uint64_t* sr_seed, costa_comm_t comm, void* stream);
/* the op of mx_dual_kernel: output 1 exactly as costa_hip_execute_tiles_mx takes it, and where source
 * element (f, s) goes in output 2, whose element has target coordinates (j, i) and whose F_ROWS is the
 * complement of the op's */
typedef struct {
    costa_scaled_op_t s; /* output 1 */
    uint64_t dst2;       /* output 2: byte offset added to dst2_base (absolute when the base is NULL) */
    int32_t ldd2;        /* elements */
    uint32_t flags2;     /* COSTA_TILE_TRANSPOSE: dst2(f*ldd2 + s), else dst2(s*ldd2 + f); the library
                            sets COSTA_TILE_VEC_DST */
} costa_dual_op_t; /* 64 bytes */
/* dual ops of COSTA_FLOAT -> dst_dtype in ONE launch of mx_dual_kernel; fp32 scalars.  m x n is output
 * 1's matrix (c_scales is indexed by it, ct_scales by the n x m one).  The per-op checks run on the
 * ops: the block rule and the packed rules on both outputs, kind not AXPBY.  sr_seed as above. */
int costa_hip_execute_tiles_mx_dual(costa_dtype_t dst_dtype, const costa_dual_op_t* ops, int64_t n_ops,
                                    const void* src_base, void* dst_base, void* dst2_base,
                                    const void* scalars, int n_slots, const costa_mx_scales_t* c_scales,
                                    const costa_mx_scales_t* ct_scales, int rounding, int64_t m, int64_t n,
                                    const uint64_t* sr_seed, int device);
/* sub-tiles run by mx_dual_kernel since the last reset (costa_hip_mx_items does not count them) */
int costa_hip_mx_dual_items(int64_t* items, int reset);
/* (costa_hip_plan_export_dual, host only: below, with the other plan exports) */

/* ---- Block-scaled FP8 transforms (fp32 scales) (MI355X-native): 1 x 128 / 128 x 128 blocks, fused ----
 * FP8 data with one fp32 scale per 1 x 128 group of a row, 128 x 1 group of a column or 128 x 128
 * tile ("blockwise" / DeepSeek-style scaling), produced or consumed in the pass that redistributes
 * or transposes.
 *
 * Scale tensor.  A DEVICE array of fp32 described by costa_block_scales_t.  Block (bi, bj) covers rows
 * bi*block_rows .. and columns bj*block_cols .. of the layout's matrix; its scale is
 * ((float*)data)[bi*row_stride + bj*col_stride] (strides count floats).  The block shapes are (1, 128),
 * (128, 1) and (128, 128); any other is COSTA_ERR_ARG.  The last block along either dimension may be
 * partial and reduces over the elements that exist.  Both strides must be positive, no two blocks of
 * the matrix may share a float, data must be 4-byte aligned.  As in the MX calls, a_scales is indexed by
 * A's matrix as stored (before trans), c_scales by C's matrix.
 *
 * Arithmetic (bit-exact).  w() / cvt() are the FP8 codecs, g() the ZERO / ALPHA / AXPBY arithmetic in
 * fp32 with contraction off.  Per element x = w(a), times SA[block of a] when A is FP8 (one rounded
 * fp32 product); v = g(x, w(c_old)).
 *   dequantise (no c_scales): store v.
 *   quantise / requantise, per block of C: amax = the unsigned maximum of the bit patterns of |v|.  If
 *     its exponent field is 255 (an inf or a NaN in the block) S = NaN (0x7FC00000) and every
 *     q = cvt(NaN).  Otherwise amax_c = max(amax, 2^-40) (bits 0x2B800000), so S and R are finite and
 *     normal; an all-zero block stores zeros and S = 2^-40 / fmax.
 *       COSTA_BLOCK_EXACT: S = amax_c / fmax, R = fmax / amax_c, two correctly rounded fp32 divisions
 *         per block.
 *       COSTA_BLOCK_POW2: E = the MX CEIL rule applied to amax_c; S = 2^(E-127), R = 2^(127-E), exact.
 *     q = cvt(clamp(v * R, -fmax, +fmax)) (one rounded product per element; under EXACT amax * R may
 *     round above fmax, so the clamp matters); SC[block] = S.  fmax is 448 (e4m3) / 57344 (e5m2).
 *
 * Accepted calls (everything else is COSTA_ERR_ARG naming what was wrong, C and the tensors untouched):
 *   quantise    COSTA_FLOAT -> FP8      c_scales           beta = 0
 *   dequantise  FP8 -> COSTA_FLOAT      a_scales           alpha, beta free
 *   requantise  FP8 -> the same FP8     both (shapes may differ)   beta = 0
 * FP8 is COSTA_FP8_E4M3 or COSTA_FP8_E5M2.  Refused: every other pair ("no block-scaled transform",
 * naming both types), a missing or superfluous descriptor, an unknown rounding value, a triangular
 * mask, an in-place call, a host-resident layout or tensor.
 *
 * Tile-boundary rule.  A block of C must not be split between tiles: every split point of both
 * layouts (A's seen through trans) must be a multiple of c_scales.block_rows along rows and of
 * c_scales.block_cols along columns (an extent of 1 holds trivially).  A violation is COSTA_ERR_ARG
 * containing "scale block" and the offending interval, raised before anything is written.  a_scales
 * imposes no rule: any layout pair dequantises.
 *
 * Several ranks: as for MX.  The exchange is the ordinary scaled plan of the FP8 pair (fp32 -> Q sends
 * fp32 and quantises in UNPACK; Q -> .. sends Q bytes); only LOCAL and UNPACK touch scale tensors.  A
 * rank writes only the scales of blocks it owns in C (zero the tensor and merge with all_reduce(MAX));
 * it needs the a_scales of every block it reads -- the library moves no scales.
 *
 * Not covered: bf16 / fp16 sides, other block sizes, packed types, batches, masks, in-place calls, host
 * staging, swizzled scales, the C++ overloads and ScaLAPACK shims. */
#define COSTA_BLOCK_EXACT 0
#define COSTA_BLOCK_POW2 1
typedef struct {
    void* data;                     /* device array of fp32 */
    int32_t block_rows, block_cols; /* (1, 128), (128, 1) or (128, 128) */
    int64_t row_stride, col_stride; /* floats between vertically / horizontally adjacent blocks */
} costa_block_scales_t; /* 32 bytes */
int costa_hip_transform_block_scaled(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                     const void* beta, const costa_block_scales_t* a_scales,
                                     const costa_block_scales_t* c_scales, int rounding, costa_comm_t comm);
int costa_hip_transform_block_scaled_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                           const void* beta, const costa_block_scales_t* a_scales,
                                           const costa_block_scales_t* c_scales, int rounding,
                                           costa_comm_t comm, void* stream);
/* ops as for costa_hip_execute_tiles_mx: m x n is C's matrix, a_transposed: A's matrix is n x m and
 * a_scales is indexed by it; with c_scales the ops obey the tile-boundary rule and have beta = 0 */
int costa_hip_execute_tiles_block_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                         const costa_scaled_op_t* ops, int64_t n_ops, const void* src_base,
                                         void* dst_base, const void* scalars, int n_slots,
                                         const costa_block_scales_t* a_scales,
                                         const costa_block_scales_t* c_scales, int rounding, int64_t m,
                                         int64_t n, int a_transposed, int device);
/* work items run by the block-scaled kernels since the last reset: 64 x 64 sub-tiles of dequantising
 * lists, 128 x 128 regions of quantising ones */
int costa_hip_block_items(int64_t* items, int reset);
/* host only: the tile-boundary rule on caller-given ops / the checks of a descriptor */
int costa_hip_block_check_ops(const costa_scaled_op_t* ops, int64_t n_ops, int block_rows, int block_cols,
                              int64_t m, int64_t n);
int costa_hip_block_check_scales(const costa_block_scales_t* desc, int64_t rows, int64_t cols);

/* ---- stream-ordered variants (MI355X-native; no reference counterpart) ----
 * Enqueue the transform and return.  Layouts must be device-resident.  `stream` (a hipStream_t,
 * may be NULL) is joined at entry and made to wait for the result, so work queued on it after
 * this call sees sub(C) complete.  Transforms of one process run in call order.
 * costa_hip_synchronize waits for everything queued on the communicator's device. */
int costa_hip_transform_async(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                              const void* beta, costa_comm_t comm, void* stream);
int costa_hip_transform_batch_async(int n, const costa_layout_t* A, const costa_layout_t* C,
                                    const char* trans, const void* alpha, const void* beta,
                                    costa_comm_t comm, void* stream);
int costa_hip_synchronize(costa_comm_t comm);

/* ---- direct tile entry points (device pointers) ---- */
int costa_hip_copy_and_transform(costa_dtype_t dtype, int n_rows, int n_cols, const void* src,
                                 int src_stride, int src_col_major, void* dst, int dst_stride,
                                 int dst_col_major, int transpose, int conjugate,
                                 const void* alpha, const void* beta);
/* runs `n` tile ops in ONE batched launch; `scalars` = n_slots (alpha, beta) pairs (host) */
int costa_hip_execute_tiles(costa_dtype_t dtype, const costa_tile_op_t* ops, int64_t n,
                            const void* src_base, void* dst_base, const void* scalars,
                            int n_slots, int device);
/* the same for converting ops: sources hold src_dtype, destinations dst_dtype (a mixed pair as
 * above), dst = g(convert(src)); offsets and leading dimensions of each side count in that side's
 * elements / bytes as in costa_tile_op_t; `scalars` = n_slots (alpha, beta) pairs of dst_dtype.
 * COSTA_SCALE_BITCOPY means "convert only" here (never a byte copy).  The VEC flags are recomputed
 * from each side's actual address: the side of the wider type takes 16-byte vector accesses when
 * 16-byte aligned, the other side 8-byte ones when 8-byte aligned.
 * Half-precision pairs ("Half precision" above: (H, H), (COSTA_FLOAT, H), (H, COSTA_FLOAT)) run
 * here too, on half_kernel: `scalars` are then n_slots (alpha, beta) pairs of fp32, a 2-byte side
 * takes 8-byte vector accesses when 8-byte aligned, an fp32 side 16-byte ones when 16-byte aligned,
 * and COSTA_SCALE_BITCOPY of an (H, H) op is a byte copy.
 * FP8 pairs ("FP8" above: (Q, Q), (COSTA_FLOAT, Q), (Q, COSTA_FLOAT)) run here on fp8_kernel, with
 * fp32 `scalars`: both sides of a (Q, Q) op take vector accesses when 16-byte aligned; next to an
 * fp32 side (16-byte aligned) a 1-byte side takes 4-byte ones when 4-byte aligned; and
 * COSTA_SCALE_BITCOPY of a (Q, Q) op is a byte copy. */
int costa_hip_execute_tiles_mixed(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                  const costa_tile_op_t* ops, int64_t n, const void* src_base,
                                  void* dst_base, const void* scalars, int n_slots, int device);
/* the sub-tile one workgroup of the converting kernels runs for a mixed, half-precision or FP8 pair
 * ((H, H) and (Q, Q) included): elements along the source's fast (*bf) and slow (*bs) dimension */
int costa_hip_convert_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs);

/* edge ops (costa_tri_op_t) of one dtype in ONE launch of tri_kernel; the VEC flags are recomputed
 * from each side's actual address */
int costa_hip_execute_tiles_tri(costa_dtype_t dtype, const costa_tri_op_t* ops, int64_t n,
                                const void* src_base, void* dst_base, const void* scalars,
                                int n_slots, int device);
/* rows of the bands the planner cuts a tile crossing the mask's diagonal into */
int costa_hip_tri_cut(void);
/* the sub-tile one workgroup of tri_kernel runs: elements along the source's fast (*bf) and slow
 * (*bs) dimension */
int costa_hip_tri_subtile(costa_dtype_t dtype, int* bf, int* bs);

/* scaled ops (costa_scaled_op_t) of one accepted pair ("scaled transforms" above) in ONE launch of
 * scaled_kernel: offsets and leading dimensions of each side count in that side's elements / bytes,
 * `scalars` = n_slots (alpha, beta) pairs of the compute type (host), `row_scale` / `col_scale`
 * device arrays of the compute type indexed by the ops' target coordinates (either may be NULL,
 * not both).  The VEC flags are recomputed from each side's actual address: a side takes vector
 * accesses when it is aligned to its strip of 4 elements (4 bytes on a 1-byte side, 8 on a 2-byte
 * side, 16 on fp32 and -- two accesses -- on fp64). */
int costa_hip_execute_tiles_scaled(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                   const costa_scaled_op_t* ops, int64_t n, const void* src_base,
                                   void* dst_base, const void* scalars, int n_slots,
                                   const void* row_scale, const void* col_scale, int device);
/* the sub-tile one workgroup of scaled_kernel runs for an accepted pair: elements along the
 * source's fast (*bf) and slow (*bs) dimension */
int costa_hip_scaled_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs);
/* ... of an MX pair (costa_hip_transform_mx) and of a block-scaled pair
 * (costa_hip_transform_block_scaled: the 128 x 128 regions of a quantising pair) */
int costa_hip_mx_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs);
int costa_hip_block_subtile(costa_dtype_t src_dtype, costa_dtype_t dst_dtype, int* bf, int* bs);
/* sub-tiles run by scaled_kernel since the last reset (scaled transforms and
 * costa_hip_execute_tiles_scaled); kept beside costa_stats_t, whose layout does not change */
int costa_hip_scaled_items(int64_t* items, int reset);
/* costa_hip_execute_tiles_scaled plus the amax outputs ("amax outputs" above): `row_amax` /
 * `col_amax` are device arrays of the compute type indexed by the ops' target coordinates (either
 * may be NULL, not both) and updated with every op's source values; the scales may both be NULL */
int costa_hip_execute_tiles_amax(costa_dtype_t src_dtype, costa_dtype_t dst_dtype,
                                 const costa_scaled_op_t* ops, int64_t n, const void* src_base,
                                 void* dst_base, const void* scalars, int n_slots,
                                 const void* row_scale, const void* col_scale, void* row_amax,
                                 void* col_amax, int device);
/* sub-tiles run by the AMAX instantiations of scaled_kernel (amax transforms and
 * costa_hip_execute_tiles_amax) and by the reduce-only kernel of costa_hip_layout_amax since the
 * last reset; kept beside costa_stats_t.  costa_hip_scaled_items keeps counting every scaled_kernel
 * sub-tile, those of the AMAX instantiations included */
int costa_hip_amax_items(int64_t* items, int reset);

/* ---- plan inspection (host only, never touches a GPU) ----
 * Plans the transform for rank `rank` of `nranks` and copies the three descriptor
 * lists out.  Offsets of pack destinations / unpack sources are byte offsets into the
 * send / receive buffer; all other addresses are the layouts' own pointers.
 * The package element size is that of the layouts' dtype; for a mixed pair (A and C of different
 * dtypes) it is the smaller of the two: pack ops then read A's type and write the package type,
 * unpack ops read the package type and write C's, local ops read A's and write C's, and each
 * side's byte offsets and VEC flag follow its own element size.  Counts and displacements are in
 * elements; `scalars` are of C's dtype -- of the compute type COSTA_FLOAT (fp32) when A or C is a
 * 2-byte type, whose package holds the 2-byte type, or a 1-byte type, whose package holds A's type.
 * Call once with NULL arrays to get the sizes in *info, then again with arrays of
 * at least those sizes. */
typedef struct {
    int64_t n_local;     /* local tile ops   (copy_local_blocks)           */
    int64_t n_pack;      /* pack tile ops    (copy_to_buffer)              */
    int64_t n_unpack;    /* unpack tile ops  (copy_from_buffer)            */
    int64_t send_elems;  /* elements in the send buffer                    */
    int64_t recv_elems;  /* elements in the receive buffer                 */
    int64_t local_elems; /* elements moved by local ops                    */
    int32_t n_ranks;     /* size of the counts/displacement arrays         */
    int32_t n_slots;     /* number of (alpha, beta) pairs                  */
} costa_plan_info_t;

int costa_hip_plan_export(int n, const costa_layout_t* A, const costa_layout_t* C,
                          const char* trans, const void* alpha, const void* beta, int rank,
                          int nranks, costa_plan_info_t* info, costa_tile_op_t* local_ops,
                          costa_tile_op_t* pack_ops, costa_tile_op_t* unpack_ops,
                          int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                          int64_t* recv_displs, void* scalars);

/* The plan of a triangular transform (costa_hip_transform_tri): the ordinary lists hold the tiles
 * wholly inside the mask (and the dense pack ops of edge tiles), local_tri / unpack_tri the edge
 * tiles that write C. */
typedef struct {
    costa_plan_info_t base;
    int64_t n_local_tri;
    int64_t n_unpack_tri;
} costa_tri_plan_info_t;
int costa_hip_plan_export_tri(costa_layout_t A, costa_layout_t C, char trans, char uplo, int k,
                              const void* alpha, const void* beta, int rank, int nranks,
                              costa_tri_plan_info_t* info, costa_tile_op_t* local_ops,
                              costa_tile_op_t* pack_ops, costa_tile_op_t* unpack_ops,
                              costa_tri_op_t* local_tri, costa_tri_op_t* unpack_tri,
                              int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                              int64_t* recv_displs, void* scalars);

/* The plan of a scaled transform (costa_hip_transform_scaled): tile set, order, pack list, package
 * type, counts, displacements and scalars are the ordinary plan's (costa_hip_plan_export), byte for
 * byte; every LOCAL and UNPACK op is in local_scaled / unpack_scaled with its target coordinates
 * (the ordinary op plus COSTA_SCALED_F_ROWS where it applies), and the ordinary local / unpack
 * lists are empty (base.n_local = base.n_unpack = 0).  `scalars` are of the compute type. */
typedef struct {
    costa_plan_info_t base;
    int64_t n_local_scaled;
    int64_t n_unpack_scaled;
} costa_scaled_plan_info_t;
int costa_hip_plan_export_scaled(costa_layout_t A, costa_layout_t C, char trans, const void* alpha,
                                 const void* beta, int rank, int nranks,
                                 costa_scaled_plan_info_t* info, costa_tile_op_t* pack_ops,
                                 costa_scaled_op_t* local_scaled, costa_scaled_op_t* unpack_scaled,
                                 int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                                 int64_t* recv_displs, void* scalars);
/* ... and of a dual-output MX quantise ("Dual-output MX quantise"): the LOCAL and UNPACK dual ops of
 * `rank`, in the order of costa_hip_plan_export_scaled(A, C, trans), whose pack ops, counts and
 * scalars are the call's.  A first call with NULL arrays returns the counts in
 * info->n_local_scaled / n_unpack_scaled; the twin rule, both block rules (with c_axis / ct_axis,
 * COSTA_MX_ROWS or COSTA_MX_COLS; -1: not checked) and the packed rules raise their errors. */
int costa_hip_plan_export_dual(costa_layout_t A, costa_layout_t C, costa_layout_t Ct, char trans,
                               const void* alpha, int c_axis, int ct_axis, int rank, int nranks,
                               costa_scaled_plan_info_t* info, costa_dual_op_t* local_dual,
                               costa_dual_op_t* unpack_dual);

/* ---- measurement ----
 * With profiling on, every kernel launch and exchange is bracketed by HIP events on
 * the stream it runs on; the sums are read (and optionally reset) here. */
typedef struct {
    double pack_ms, local_ms, unpack_ms, exchange_ms, h2d_ms, d2h_ms;
    int64_t pack_launches, local_launches, unpack_launches;
    int64_t pack_bytes, local_bytes, unpack_bytes; /* algorithmic HBM bytes */
    int64_t transforms;
    int64_t plan_hits, plan_misses;
    int64_t host_groups; /* tile groups moved by the pipelined host staging */
    int64_t device_plans; /* plan-cache misses planned on the GPU (costa_hip_set_planner) */
    double plan_ms;       /* host wall time spent building plans (cache misses) */
    int64_t host_direct;  /* host-resident calls whose buffers were page-locked and in which some
                             tile groups moved by strided DMA between the caller's memory and
                             HBM (no host copies for those groups) */
    int64_t host_direct_groups; /* ... the tile groups that moved that way (PACK: a pack kernel
                                   from the DMA'd source rectangle; LOCAL / UNPACK: kernels
                                   writing the target rectangle's image, DMA'd back) */
    /* work items launched by the device-resident path, per kernel (r6): tile_kernel sub-tiles
       (the large, square, medium and 32 x 32 shapes), skew_kernel sub-tiles, cblock_kernel
       destination-block groups, tiny_kernel wavefront pieces */
    int64_t tile_items, skew_items, cblock_items, tiny_items;
    int64_t device_lists; /* work lists whose destination-block groups were built on the GPU
                             (costa_hip_set_list_builder) */
    int64_t fused_pieces; /* of tiny_items: wavefront pieces run as workgroups at the end of the
                             destination-block group launch (no tiny_kernel launch of their own) */
    int64_t convert_items; /* sub-tiles run by convert_kernel, half_kernel and fp8_kernel (the
                              converting lists of mixed, half-precision and FP8 transforms,
                              costa_hip_execute_tiles_mixed) */
    int64_t tri_items; /* sub-tiles run by tri_kernel (the edge tiles of triangular transforms,
                          costa_hip_execute_tiles_tri) */
} costa_stats_t;
/* of local_ms + unpack_ms: the event time of the edge-tile launches of triangular transforms since
 * the last reset (their share of a masked call, tools/bench_tri.py) */
int costa_hip_tri_phase_ms(double* ms, int reset);
int costa_hip_set_profiling(int on);
int costa_hip_get_stats(costa_stats_t* out, int reset);
/* drop cached plans and device workspaces of this process */
int costa_hip_release_caches(void);

/* ---- host-resident layouts ----
 * How a transform whose layouts live in host memory reaches HBM (the reference's path starts
 * and ends in each rank's host buffers).  1 (default; env COSTA_HOST_STAGING): pipelined --
 * the tiles move in 64 MiB groups through pinned/device slot rings: host gather -> H2D ->
 * tile kernels -> D2H -> host scatter, both copy directions at once; with several ranks the
 * host gather writes the send package, the RCCL exchange follows, and the unpack kernels'
 * output comes back the same way.  When every host buffer of the call is page-locked
 * (hipHostMalloc, or registered by the caller with hipHostRegister) the pipeline skips the host
 * copies: each tile moves by strided DMA (hipMemcpy2DAsync) straight between the caller's memory
 * and the device slots, both directions at once.  0: mirror -- every byte range the layouts span is uploaded,
 * the kernels run on the mirror, the target ranges are copied back.  Mode 1 falls back to 0
 * for in-place layouts and target ranges shared by two batched jobs.  Results are identical. */
int costa_hip_set_host_staging(int mode);

/* Planner of plan-cache misses (the reference plans on the host at every call, utils.hpp:87-206,
 * communication_data.cpp:67-164).  1 (default): layout pairs of at least 4096 blocks are planned
 * on the GPU (100000 before the first GPU plan of the process, which loads the planner's kernels)
 * -- one thread per cell of the merged grid of the two layouts, a stable radix sort by
 * peer for the message order, scans for the package offsets; 0: always on the host; 2: on the GPU
 * wherever it applies.  The op lists are identical either way.  Layouts whose local blocks are
 * not exactly the rank's grid cells are planned on the host in every mode. */
int costa_hip_set_planner(int mode);
/* costa_hip_plan_export through the GPU planner of `device` (COSTA_ERR_ARG when it does not
 * apply to these layouts) */
int costa_hip_plan_export_device(int device, int n, const costa_layout_t* A, const costa_layout_t* C,
                                 const char* trans, const void* alpha, const void* beta, int rank,
                                 int nranks, costa_plan_info_t* info, costa_tile_op_t* local_ops,
                                 costa_tile_op_t* pack_ops, costa_tile_op_t* unpack_ops,
                                 int64_t* send_counts, int64_t* send_displs, int64_t* recv_counts,
                                 int64_t* recv_displs, void* scalars);

/* Builder of the executor's work lists on a plan-cache miss (after the planner): the
 * destination-block groups of the wavefront ops -- components of ops that tile a destination
 * range exactly, cut into column bands, in destination / XCD-slice order -- are 1 (default) built
 * on the GPU for lists of at least 16384 wavefront ops, 0 always on the host, 2 on the GPU wherever
 * they apply (env COSTA_LIST_BUILDER).  The lists are identical either way. */
int costa_hip_set_list_builder(int mode);
/* The executor's work lists of one tile-op list (diagnostics and tests; no kernel runs):
 * `kind` 0 local, 1 pack (destination = a dense package), 2 unpack; device < 0 builds them on the
 * host, device >= 0 with the destination-block groups on that GPU.  meta[12] receives n_large,
 * n_medium, n_skew, n_cblock, cblock_lds, cb_map, tiny_first, n_tiny, n_ordered, n_work, whether the
 * GPU built part of them, and the flags (bit 0 tr_shape, 1 sq, 2 full, 3 med_full, 4 med_sq,
 * 5 skew_wide).  `ordered` (cap_ordered ops) and `work` (cap_work entries) are filled when their
 * capacities suffice (NULL: sizes only). */
int costa_hip_work_export(int dtype, const costa_tile_op_t* ops, int64_t n_ops, int kind, int device,
                          costa_tile_op_t* ordered, int64_t cap_ordered, uint64_t* work,
                          int64_t cap_work, int64_t* meta);

#ifdef __cplusplus
}
#endif
#endif /* COSTA_HIP_H */
