/*
 * subspace_hip.h — C ABI of libsubspace_hip.so, the MI355X (gfx950) implementation of the
 * subspace linear-algebra hot path of molpro::linalg::itsolv.
 *
 * Every entry point replaces one operation of the reference's ArrayHandler interface
 * (reference: src/molpro/linalg/array/ArrayHandler.h:184-222) acting on the LOCAL shard of
 * HBM-resident vectors, plus the MPI_Allreduce the reference's distributed handlers issue
 * after local reductions (src/molpro/linalg/array/util/gemm.h:179-182, DistrArray.cpp:134-136).
 *
 * Conventions:
 *  - All vector arguments are DEVICE pointers (double, FP64) of the calling rank's shard of
 *    length n; they must be 16-byte aligned (ssp_alloc guarantees 256 B).
 *  - Matrices are row-major, as subspace::Matrix is (reference itsolv/subspace/Matrix.h:23):
 *      gemm_inner: out[i*k + j] = <xx[i], yy[j]>            (reference util/gemm.h:267-279)
 *      gemm_outer: yy[j] += sum_i alphas[i*m + j] * xx[i]   (reference util/gemm.h:257-265)
 *  - Ops are ordered on the context's HIP stream.  Ops that return host values (dot,
 *    gemm_inner, select, sparse dot/gemm_inner) synchronise that stream before returning.
 *  - With a communicator attached (ssp_ctx_attach_comm), reductions are summed over ranks with
 *    RCCL allreduce on the same stream, so every rank receives bit-identical results.
 *  - No entry point throws.  Each returns an ssp_status; ssp_last_error() describes the last
 *    failure on the calling thread.  The C++ handler shim maps codes to the reference's
 *    exceptions (ArrayHandlerError, std::out_of_range, std::logic_error).
 */
#ifndef SUBSPACE_HIP_H
#define SUBSPACE_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  SSP_OK = 0,
  SSP_ERR_SIZE = 1,      /* incompatible vector sizes  -> util::ArrayHandlerError   */
  SSP_ERR_RANGE = 2,     /* matrix/vector count mismatch -> std::out_of_range       */
  SSP_ERR_ARG = 3,       /* invalid argument (null, misaligned, n too large)         */
  SSP_ERR_HIP = 4,       /* HIP runtime failure                                      */
  SSP_ERR_COMM = 5,      /* RCCL failure                                             */
  SSP_ERR_NOMEM = 6,     /* device or pinned allocation failed                      */
  SSP_ERR_UNSUPPORTED = 7, /* operation not defined for these operands -> logic_error */
  SSP_ERR_COMM_ABANDONED = 8 /* an RCCL join of this process was abandoned at its deadline: no further
                                RCCL attach in this process (end it); the host-callback and peer-memory
                                transports stay available */
} ssp_status;

typedef struct ssp_ctx ssp_ctx;

/* ---- context, memory, communicator ------------------------------------------------------ */
const char* ssp_last_error(void);
const char* ssp_version(void);
/* Number of visible HIP devices (0 when no GPU).  Does not create a context. */
int ssp_device_count(void);
int ssp_ctx_create(int device, ssp_ctx** out);
int ssp_ctx_destroy(ssp_ctx* ctx);
/* The hipStream_t all ops of this context run on (for event timing by callers, and for their own
 * kernels on the library's vectors).  Stores every deferred zero fill (ssp_fill) first: call it, or
 * ssp_synchronize, AFTER the library calls whose results foreign code is going to read -- a stream
 * handle taken earlier does not order foreign work behind a fill that was deferred later. */
void* ssp_ctx_stream(ssp_ctx* ctx);
/* Stores every deferred zero fill, then waits until the stream is idle. */
int ssp_synchronize(ssp_ctx* ctx);
/* Caching device allocator (HBM arena): Q vectors are created and destroyed every iteration
 * (reference itsolv/subspace/QSpace.h:80-84), so freed blocks are recycled by size. */
int ssp_alloc(ssp_ctx* ctx, size_t n, double** out);
int ssp_free(ssp_ctx* ctx, double* p);
int ssp_release_cached(ssp_ctx* ctx);
int ssp_memory_stats(ssp_ctx* ctx, size_t* bytes_in_use, size_t* bytes_cached);
int ssp_upload(ssp_ctx* ctx, double* dst_dev, const double* src_host, size_t n);
int ssp_download(ssp_ctx* ctx, double* dst_host, const double* src_dev, size_t n);

/* RCCL communicator over one process per GPU.  The id is SSP_UNIQUE_ID_BYTES opaque bytes made
 * by rank 0 with ssp_comm_unique_id and distributed by the caller (e.g. torch.distributed). */
#define SSP_UNIQUE_ID_BYTES 128
int ssp_comm_unique_id(char* id_out);
/* Collective: returns once every rank has joined, SSP_ERR_COMM when RCCL reports the join failed, or
 * SSP_ERR_COMM_ABANDONED when the communicator has not formed within the communication deadline
 * (ssp_ctx_set_comm_timeout; a rank is missing).  An abandoned join leaves its helper thread inside
 * RCCL's bootstrap, so every later ssp_ctx_attach_comm of the process returns SSP_ERR_COMM_ABANDONED at
 * once: do not retry -- end the process, or attach the host-callback / peer-memory transport. */
int ssp_ctx_attach_comm(ssp_ctx* ctx, int nranks, int rank, const char* id);
int ssp_ctx_rank(ssp_ctx* ctx);
int ssp_ctx_nranks(ssp_ctx* ctx);
/* In-place sum over ranks of n doubles in DEVICE memory (no-op without a communicator). */
int ssp_allreduce_sum(ssp_ctx* ctx, double* buf_dev, size_t n);
/* Gather `bytes` host bytes from every rank into recv (nranks*bytes), rank order. */
int ssp_allgather_host(ssp_ctx* ctx, const void* send, void* recv, size_t bytes);
/* Host-callback communicator in place of RCCL: reductions are staged through host memory and
 * handed to the callbacks (return 0 on success).  For transports without RCCL and for testing
 * the sharded path with several ranks on one device.  Replaces any attached RCCL communicator. */
typedef int (*ssp_host_allreduce_fn)(double* buf, size_t n, void* user);
typedef int (*ssp_host_allgather_fn)(const void* send, void* recv, size_t bytes, void* user);
int ssp_ctx_attach_host_comm(ssp_ctx* ctx, int nranks, int rank, ssp_host_allreduce_fn allreduce,
                             ssp_host_allgather_fn allgather, void* user);
/* Peer-memory communicator (no RCCL): the ranks of ONE node exchange reduction partials through
 * IPC-shared device memory (push into every rank's inbox, device-side flag wait, fixed rank-order
 * sum: bit-identical results on every rank) and host data through a POSIX shared-memory segment.
 * Several ranks may share one device.  `id` (SSP_UNIQUE_ID_BYTES, from ssp_p2p_unique_id on rank 0)
 * is distributed by the caller.  Collective: returns once every rank has attached.  At most 16 ranks.
 * Replaces any other communicator. */
int ssp_p2p_unique_id(char* id_out);
int ssp_ctx_attach_p2p(ssp_ctx* ctx, int nranks, int rank, const char* id);
/* Fail fast: every wait that depends on other ranks gives up after `seconds` (default 300, or
 * SSP_COMM_TIMEOUT_S at context creation), and RCCL's asynchronous errors are polled meanwhile; the
 * communicator is then aborted (ncclCommAbort / the peer-memory abort word) and the call, and every
 * later exchange on the context, returns SSP_ERR_COMM naming the operation -- the status-code form of
 * the reference's abort of the whole job on a distributed error (DistrArray.cpp:16-23). */
int ssp_ctx_set_comm_timeout(ssp_ctx* ctx, double seconds);
/* Vectors of at most n local elements (default 2048, or SSP_EXACT_MAX at context creation; 0 turns
 * it off; attaching a communicator gives every rank the smallest value among the ranks, and a later
 * call must pass the same n on every rank) are computed in the reference's own arithmetic: every dot a sequential sum in index order
 * (std::inner_product, ArrayHandlerIterable.h:76-82) and every y = alpha x + y rounded twice (no fused
 * multiply-add, ArrayHandlerIterable.h:65-74), gemm_inner / gemm_outer pairwise in the reference's loop
 * order (util/gemm.h:257-279), fused entry points as their documented unfused sequence.  Results on
 * such vectors are the reference CPU path's bit for bit; longer vectors use the bandwidth kernels.
 * Sharded, the choice is each rank's on its own shard length: when the global length puts the
 * longer shards (make_distribution_spread_remainder lengths differ by one) just above n and the
 * shorter ones at n, the ranks' partials come from both arithmetics -- in the same result layout,
 * summed as always, every rank receiving the same sums -- and the bit-for-bit claim is then void. */
int ssp_ctx_set_exact_max(ssp_ctx* ctx, size_t n);
/* Shard of a global length n owned by `rank` of `nranks` (host only, no context):
 * make_distribution_spread_remainder, reference util/Distribution.h:99-109. */
int ssp_shard_range(size_t n, int nranks, int rank, size_t* offset, size_t* length);

/* Operation ledger (measurement): when enabled, HIP events on the
 * context's stream bracket each hot-path kernel launch and the call's ALGORITHMIC bytes are
 * accumulated per operation name ("gemm_inner", "gemm_outer", "axpy", "dot", ...). */
int ssp_ledger_enable(ssp_ctx* ctx, int enable);
int ssp_ledger_reset(ssp_ctx* ctx);
int ssp_ledger_count(ssp_ctx* ctx);
/* Pre-create n ledger events (2 per recorded op), so that a ledger over a timed region creates none. */
int ssp_ledger_reserve(ssp_ctx* ctx, int n);
int ssp_ledger_entry(ssp_ctx* ctx, int i, const char** name, long long* calls, double* kernel_ms, double* bytes);

/* ---- dense (R x R, Q x Q, R x Q) operations: reference ArrayHandlerIterable.h:46-90,
 *      DistrArray.cpp:43-138 ------------------------------------------------------------- */
/* x[:] = alpha                         reference ArrayHandlerIterable.h:59-63
 * A fill with +0.0 of a vector longer than exact_max is deferred: the call launches nothing and the
 * library remembers the range (up to 64 of them).  Every later entry point of the context first stores
 * the remembered zeros (one fill kernel each, in the order of the calls), so every library call, copy
 * and reduction sees exactly the memory an immediate fill would have left, with these exceptions that
 * do less work for the same bits:
 *   ssp_gemm_outer[_scaled]  whose destinations are all exactly deferred vectors (same address and
 *                            length, none twice, no destination scale): runs as ssp_gemm_outer_set, the
 *                            zeros are never written or read (fill(0) + gemm_outer in one write-only
 *                            pass, the reference's construct_solution); otherwise the fills of its
 *                            operands are stored first and it runs read-modify-write;
 *   ssp_gemm_outer_set[_scaled], ssp_copy, ssp_scal_copy, another ssp_fill
 *                            that overwrite a deferred vector whole: its zeros are never written;
 *   ssp_free                 of the block that holds it: likewise.
 * Deferred fills that a call does not touch stay deferred across these.  Code that reads device
 * memory WITHOUT a library call (its own kernels, hipMemcpy) must take ssp_ctx_stream or call
 * ssp_synchronize after the fill.  -0.0, non-zero values and short vectors are filled at once.
 * Lifetime: the zeros may be written at any later entry point of the context, so memory the library
 * did not allocate (a vector over the caller's own hipMalloc block, from C, Fortran or a non-owning
 * view) must stay allocated until a call that stores or drops the fill -- any call other than the
 * exceptions above, ssp_ctx_stream or ssp_synchronize -- has returned; blocks of ssp_alloc are safe,
 * ssp_free drops their fills.
 * SSP_DEFER_FILL=0 in the environment at ssp_ctx_create: every fill is launched at once.
 *
 * Deferred gemm_outer.  A write-only gemm_outer -- ssp_gemm_outer_set[_scaled], or ssp_gemm_outer[_scaled]
 * that ran as one over deferred vectors (above) -- with every scale 1.0, at most 64 sources and 16
 * destinations and vectors longer than the short-vector limit is validated at once but launched LATER:
 * by the next entry point of the context, whichever it is, before that entry point does anything else.
 * Errors of the arguments are reported by the call itself, a failure of the launch by the call that
 * launches it.  The one exception: an ssp_axpy (or ssp_axpy_scaled with both scales 1.0) whose y is
 * exactly one of the pending destinations (same address and length), that has no such axpy yet, and
 * whose x shares no byte with any pending destination (it may be one of the sources), with
 * sources + destinations <= 64.  It launches nothing: the pending launch adds alpha * x to that
 * destination's finished sum before storing it, by the fma the axpy itself would have applied to the
 * stored value, so the results are the same bits with one read and one write of y less (the residual
 * update r_i -= lambda_i x_i after construct_solution).  It is the same contract as for deferred fills:
 * every library call sees the memory the immediate launches would have left; code that touches device
 * memory WITHOUT a library call must take ssp_ctx_stream or call ssp_synchronize first, and the
 * operands (x of an attached axpy included) must stay allocated until a later call of the context has
 * returned; ssp_free launches the pending gemm_outer before the block returns to the arena, and
 * ssp_ctx_destroy discards it.  In the ledger the launch is a "gemm_outer" / "gemm_outer_set" row of
 * 8 n (k + m + e) bytes for e attached terms, which have no "axpy" row.
 * When the call that launches it is ssp_dot(y, y, n) on one of at most 8 pending destinations, the launch
 * also sums the squares of every destination, and that dot and the same dot of the other destinations are
 * answered from those sums (the bits the dot itself gives, no "dot" row) until any other call of the
 * context; foreign code that writes vector memory in between must take ssp_ctx_stream or call
 * ssp_synchronize first, as above, which also drops the sums.  SSP_OUTER_NORMS=0 at ssp_ctx_create: off.
 * A second such call of the same kind (both ssp_gemm_outer over zero-filled destinations, or both
 * ssp_gemm_outer_set) with the same n, k, m <= 8 and bit-identical alphas, whose operands share no byte with
 * the first one's destinations and whose destinations share none with its sources, stays pending next to
 * it (a zero fill that touches no operand of either does not launch them).  ssp_axpy(a, x, y) with x exactly
 * destination j of the first and y exactly destination j of the second then costs no memory access at all,
 * and ssp_dot(y, y, n) on a destination of the second launches both calls as one kernel: one ledger row of
 * 2 calls and 8 n (2 k + 2 m) bytes, results bit for bit those of the separate launches.  Any other call
 * launches the first by itself and goes on as described above.  SSP_OUTER_PAIR=0 at ssp_ctx_create: off (the
 * second call launches the first).
 * SSP_DEFER_OUTER=0 in the environment at ssp_ctx_create: every gemm_outer is launched at once. */
int ssp_fill(ssp_ctx* ctx, double alpha, double* x, size_t n);
/* x[:] *= alpha                        reference ArrayHandlerIterable.h:54-57 */
int ssp_scal(ssp_ctx* ctx, double alpha, double* x, size_t n);
/* x[:] = y[:]                          reference ArrayHandlerIterable.h:48-52 */
int ssp_copy(ssp_ctx* ctx, double* x, const double* y, size_t n);
/* y[:] += alpha * x[:]                 reference ArrayHandlerIterable.h:65-74 */
int ssp_axpy(ssp_ctx* ctx, double alpha, const double* x, double* y, size_t n);
/* *out = sum_ranks <x, y>              reference ArrayHandlerIterable.h:76-82, DistrArray.cpp:124-138 */
int ssp_dot(ssp_ctx* ctx, const double* x, const double* y, size_t n, double* out);
/* out (m x k, row-major) = <xx[i], yy[j]> summed over ranks.
 * reference util/gemm.h:157-184 (distributed) and :267-279 (pairwise default) */
int ssp_gemm_inner(ssp_ctx* ctx, const double* const* xx, int m, const double* const* yy, int k, size_t n,
                   double* out);
/* yy[j] += sum_i alphas[i*m + j] * xx[i], i in [0,k) sources, j in [0,m) destinations.
 * reference util/gemm.h:186-203 (distributed) and :257-265 (pairwise default) */
int ssp_gemm_outer(ssp_ctx* ctx, const double* alphas, const double* const* xx, int k, double* const* yy, int m,
                   size_t n);
/* yy[j] = sum_i alphas[i*m + j] * xx[i]: ssp_fill(0) on every destination followed by ssp_gemm_outer,
 * bit-identical, in one pass that does not read the destinations (construct_solution,
 * reference IterativeSolverTemplate.h:33-65).  k = 0 zero-fills. */
int ssp_gemm_outer_set(ssp_ctx* ctx, const double* alphas, const double* const* xx, int k, double* const* yy, int m,
                       size_t n);
/* Fused modified-Gram-Schmidt step: yy[j] += c[j] * x, then out[j] = <yy[j], z> summed over ranks.
 * Equals ssp_gemm_outer({x} -> yy) followed by ssp_gemm_inner(yy, {z}) with bit-identical yy; one
 * pass over yy (reference propose_rspace.h:430-443 issues them as separate handler calls). */
int ssp_axpy_inner(ssp_ctx* ctx, const double* c, const double* x, double* const* yy, int m, const double* z, size_t n,
                   double* out);
/* Steps of the sequential self-orthonormalisation of the new R vectors (reference
 * propose_rspace.h:450-465: scal(1/|r_i|, r_i); for j > i: r_j -= <r_i, r_j> r_i), fused so that
 * each step is two passes:
 *   ssp_scal_inner:  x *= alpha, then out[j] = <x, yy[j]> summed over ranks   (= ssp_scal then
 *                    ssp_gemm_inner({x}, yy), x bit-identical)                 bytes 8N(2 + m)
 *   ssp_axpy_norm:   yy[j] += c[j] * x, then *out = <yy[0], yy[0]> summed over ranks (= ssp_gemm_outer
 *                    then ssp_dot(yy[0], yy[0]), yy bit-identical)             bytes 8N(1 + 2m) */
int ssp_scal_inner(ssp_ctx* ctx, double alpha, double* x, const double* const* yy, int m, size_t n, double* out);
int ssp_axpy_norm(ssp_ctx* ctx, const double* c, const double* x, double* const* yy, int m, size_t n, double* out);
/* One pass per step of that loop (the HBM handlers' default since round 3):
 *   ssp_axpy_gram:   x_s = x * xs (stored into x when store_x and xs != 1: the scal's one rounding),
 *                    yy[j] += c[j] * x_s, then out[j] = <yy[0], yy[j]> for j < m summed over ranks --
 *                    the Gram row of the next vector to normalise, from which the caller takes its
 *                    norm (out[0]) and the next overlaps <r_{i+1}, r_j> = out[j - i - 1] / |r_{i+1}|
 *                    (= ssp_gemm_outer_scaled({x} -> yy) then ssp_gemm_inner({yy[0]}, yy), yy and x
 *                    bit-identical)                                           bytes 8N(1 + store + 2m) */
int ssp_axpy_gram(ssp_ctx* ctx, const double* c, double* x, double xs, int store_x, double* const* yy, int m,
                  size_t n, double* out);
/* Block transform of m vectors in place (the block self-orthonormalisation of the new R vectors,
 * itsolv_hbm/hbm_handlers.h): x_j <- sum_{i<m} t[i*m + j] (xs_i x_i) for j < m, the outputs of each
 * element formed from its loaded inputs before any is stored (the destinations are the sources), the
 * sum by fused multiply-adds in order i = 0..m-1 (on vectors of at most exact_max elements each
 * product rounded before its add).  With gram != NULL also gram[i*m + j] = <x_i', x_j'> of the new
 * vectors (m x m, symmetric), summed over ranks, in the same pass.  1 <= m <= 8; xs may be null (all 1).
 *                                                                          bytes 16 N m */
int ssp_transform_gram(ssp_ctx* ctx, const double* t, double* const* xx, const double* xs, int m, size_t n,
                       double* gram);
/* The same transform with only the self-dots of the new vectors, norms2[j] = <x_j', x_j'> summed over
 * ranks, formed in the same pass (the M accumulators of the plain kernel's window shape; short
 * vectors: the reference's sequential dots).                               bytes 16 N m */
int ssp_transform_norms(ssp_ctx* ctx, const double* t, double* const* xx, const double* xs, int m, size_t n,
                        double* norms2);
/* Residuals and their norms (construct_residual + update_errors, reference
 * LinearEigensystemDavidson.h:186-192, IterativeSolverTemplate.h:95-102) in one pass:
 *   yy[j] = ys[j] yy[j] + c[j] (xs[j] xx[j])  (= ssp_axpy_scaled per pair, yy bit-identical),
 *   out[j] = <yy[j], yy[j]> summed over ranks.  xs / ys may be null (all 1).   bytes 24N m */
int ssp_axpy_pairs_norm(ssp_ctx* ctx, const double* c, const double* const* xx, const double* xs, double* const* yy,
                        const double* ys, int m, size_t n, double* out);
/* a[v][i] /= (d[i] - shift[v] + 1e-15) for v in [0,nvec)   reference itsolv/IterativeSolver.h:34-55 */
int ssp_precondition(ssp_ctx* ctx, double* const* a, int nvec, const double* d, const double* shift, size_t n);
/* The same with the self-dots of the results, norms2[v] = <a_v', a_v'> summed over ranks, formed in the
 * same pass (short vectors: the reference's sequential dots, as ssp_gemm_inner).  0 <= nvec <= 8.
 *                                                                          bytes 8N (1 + 2 nvec) */
int ssp_precondition_norms(ssp_ctx* ctx, double* const* a, int nvec, const double* d, const double* shift, size_t n,
                           double* norms2);

/* ---- deferred scal (itsolv_hbm/hbm_vec.h, Vec::scale_by): an operand's value is s * (its stored
 *      contents); the kernel multiplies each element by s as it loads it -- the one rounding the
 *      reference's scal loop stores -- so every *_scaled call is bit-identical to ssp_scal(s, v) on
 *      each operand v with s != 1 followed by the unscaled call, without that pass over v (16 bytes
 *      per element).  Scale arrays may be null (all 1).  A read-modify-write destination's scale
 *      (ys) applies to the values read; what is stored is the plain result.  Replaces the separate
 *      scal pass of reference ArrayHandlerIterable.h:54-57 at the call sites of propose_rspace.h:17-28
 *      and :450-465 (normalisation of the new R vectors). ------------------------------------------ */
/* x[:] = alpha * y[:]  (the stored form of a scaled vector whose block is shared) */
int ssp_scal_copy(ssp_ctx* ctx, double alpha, double* x, const double* y, size_t n);
int ssp_axpy_scaled(ssp_ctx* ctx, double alpha, const double* x, double xs, double* y, double ys, size_t n);
int ssp_dot_scaled(ssp_ctx* ctx, const double* x, double xs, const double* y, double ys, size_t n, double* out);
int ssp_gemm_inner_scaled(ssp_ctx* ctx, const double* const* xx, const double* xs, int m, const double* const* yy,
                          const double* ys, int k, size_t n, double* out);
int ssp_gemm_outer_scaled(ssp_ctx* ctx, const double* alphas, const double* const* xx, const double* xs, int k,
                          double* const* yy, const double* ys, int m, size_t n);
int ssp_gemm_outer_set_scaled(ssp_ctx* ctx, const double* alphas, const double* const* xx, const double* xs, int k,
                              double* const* yy, int m, size_t n);
int ssp_gemm_inner_sparse_scaled(ssp_ctx* ctx, const double* const* xx, const double* xs, int m, size_t n,
                                 size_t offset, const size_t* ptr, const size_t* idx, const double* val, int k,
                                 double* out);
/* The same m x k sparse inner products split in two: _begin queues them and returns at once, _end
   delivers them to out (m*k doubles).  Other calls may come in between: the subspace update
   (subspace.h new_qspace_data) queues S(R,P)/H(P,R) ahead of the dense overlap rows, so the wait for
   those rows covers both and the sparse product needs no round trip of its own.  One product may be
   pending per context: _begin discards an uncollected one, _end with nothing pending is SSP_ERR_ARG.  With a
   communicator attached (a collective) or beyond the inline limits (m > 64, k > 32, > 64 local
   entries) _begin computes the result at once. */
int ssp_gemm_inner_sparse_begin(ssp_ctx* ctx, const double* const* xx, const double* xs, int m, size_t n,
                                size_t offset, const size_t* ptr, const size_t* idx, const double* val, int k);
int ssp_gemm_inner_sparse_end(ssp_ctx* ctx, double* out);
int ssp_construct_solution_scaled(ssp_ctx* ctx, const double* palphas, const size_t* ptr, const size_t* idx,
                                  const double* val, int kp, const double* alphas, const double* const* xx,
                                  const double* xs, int k, double* const* yy, int m, size_t n, size_t offset);
/* Block update of the block Gram-Schmidt step (itsolv_hbm/rspace.h block_gram_schmidt):
 *   yy[j] = ys[j] yy[j] + sum_i palphas[i*m + j] p_i + sum_s alphas[s*m + j] xs[s] xx[s]
 * bit-identical to ssp_scal(ys) + ssp_gemm_outer_sparse (P) + ssp_gemm_outer (dense sources), in one
 * pass over the destinations (the indices the P vectors touch are recomputed in that order). */
int ssp_block_update(ssp_ctx* ctx, const double* palphas, const size_t* ptr, const size_t* idx, const double* val,
                     int kp, const double* alphas, const double* const* xx, const double* xs, int k, double* const* yy,
                     const double* ys, int m, size_t n, size_t offset);

/* ---- row blocks: a caller's row-major block of m vectors (row k at block + k*ld, any double* base and
 *      any ld >= n) into and out of library vectors, device to device, in one pass on the context's
 *      stream (csrc/kernels_rows.hip; the device forms of the reverse-communication API,
 *      include/iterative_solver_c.h, stage R through them).
 *        - The library vectors (dst[k] of the import, src[k] of the export) are 16-byte aligned like every
 *          other vector argument.  The caller's block need only be 8-byte aligned: this is the one place
 *          where the library meets memory it did not allocate, so a row may sit at 8 mod 16 (an odd ld or
 *          an odd base; with an odd ld the rows alternate).  Parity is decided per row: an aligned row
 *          moves with the 16-byte accesses of ssp_copy (window shape and nontemporal accesses from 2^24
 *          elements), a misaligned row with 8-byte accesses on both sides, lane by lane contiguous.
 *        - The import is a bit copy.  The export of a row with xs[k] == 1 (xs NULL: every row) is a bit
 *          copy; otherwise it stores the single product src[k][i] * xs[k], bit for bit ssp_scal followed
 *          by a copy (a vector's deferred scale costs no pass of its own).
 *        - Up to 16 rows go in one launch; more rows are chunked.  m = 0 or n = 0 does nothing; m < 0,
 *          ld < n, a null pointer or a misaligned library vector is SSP_ERR_ARG.
 *        - Deferred zero fills: the import's destinations are written in full (their fills are dropped),
 *          a fill recorded for a source of either call is stored first.
 *        - The caller's block must not overlap a library vector of the call (not checked).
 *      Ledger names rows_import / rows_export, 16 bytes per element and row, one entry per launch. */
/* dst[k][i] = src[k*ld + i],          k < m, i < n */
int ssp_rows_import(ssp_ctx* ctx, const double* src, size_t ld, double* const* dst, int m, size_t n);
/* dst[k*ld + i] = xs[k] * src[k][i],  xs NULL = all 1 */
int ssp_rows_export(ssp_ctx* ctx, const double* const* src, const double* xs, int m, double* dst, size_t ld, size_t n);
/* The export that rounds: dst[k*ld + i] = (double)(float)(xs[k] * src[k][i]) for k < mq, and
 * xs[k] * src[k][i] as ssp_rows_export for mq <= k < m.  The rounding is ssp_quantise_f32's (to nearest
 * even, binary32 subnormals kept, overflow to +-inf), so the bits are those of ssp_quantise_f32 on copies
 * of the first mq vectors followed by ssp_rows_export -- in one pass of 16 bytes per element and row
 * instead of 32, and the sources are not written.  The refined f32 Q space of the reverse-communication
 * API returns its new parameter rows through it (include/iterative_solver_c.h).  Same shapes, launches
 * and argument checks as ssp_rows_export; mq < 0 or mq > m is SSP_ERR_ARG.  Ledger name rows_export_q. */
int ssp_rows_export_quantised(ssp_ctx* ctx, const double* const* src, const double* xs, int m, int mq, double* dst,
                              size_t ld, size_t n);

/* ---- mixed precision: vectors STORED in binary32, all arithmetic in FP64 (csrc/kernels_mixed.hip).
 *      The Q space of a solve is written once and afterwards only read; held in f32 it takes half
 *      the HBM and half the bytes of every pass over it (itsolv_hbm/hbm_vec_f32.h).  One rule: an f32
 *      operand is widened to f64 as it is loaded (exact); the operation then performs exactly the
 *      arithmetic of its f64 entry point on the widened values; where the destination is f32 the f64
 *      result is rounded once, to nearest-even, as it is stored.  So
 *        - results into f64 destinations are bit-identical to the f64 entry point on widened operands
 *          (ssp_scal_copy, ssp_axpy, ssp_gemm_outer[_set]_scaled: the same fma chain i = 0..k-1);
 *        - results into f32 destinations are (float) of that f64 result.  Exception: ssp_mx_gemm_outer
 *          into f32 destinations with k > 64 sources runs one launch per group of 64 sources, each a
 *          read-modify-write of the f32 destinations: the sum is rounded to f32 once per group of 64;
 *        - reductions reorder the sum as the f64 kernels do (fixed order: repeated calls give the same
 *          bits) and, with a communicator attached, are summed over ranks exactly as ssp_gemm_inner's;
 *        - on vectors of at most exact_max elements (ssp_ctx_set_exact_max) axpy, dot, gemm_inner and
 *          gemm_outer widen their f32 operands into scratch f64 vectors and call the f64 entry point
 *          (the reference's arithmetic), then round f32 destinations once;
 *        - a result beyond the binary32 range becomes +/-inf on narrowing: scaling is the caller's concern;
 *        - f32 fills are never deferred, and every entry point below first stores the pending f64 zero
 *          fills of the context.
 *      All vectors of one side of a call share that side's dtype; pointers must be 16-byte aligned.
 *      (SSP_F64, SSP_F64) forwards to the f64 entry point.  Ledger names: copy_f32, axpy_f32, dot_f32,
 *      fill_f32, scal_f32, quantise_f32, gemm_inner_f32, gemm_outer_f32; bytes count 4 per f32 and 8 per f64 element. */
typedef enum { SSP_F64 = 0, SSP_F32 = 1 } ssp_dtype;
/* n floats from the arena of ssp_alloc (4 n bytes, 256-byte aligned) */
int ssp_alloc_f32(ssp_ctx* ctx, size_t n, float** out);
int ssp_free_f32(ssp_ctx* ctx, float* p);
int ssp_upload_f32(ssp_ctx* ctx, float* dst_dev, const float* src_host, size_t n);
int ssp_download_f32(ssp_ctx* ctx, float* dst_host, const float* src_dev, size_t n);
/* x[:] = (float)alpha */
int ssp_fill_f32(ssp_ctx* ctx, double alpha, float* x, size_t n);
/* x[:] = (float)(alpha * (double)x[:]) */
int ssp_scal_f32(ssp_ctx* ctx, double alpha, float* x, size_t n);
/* x[:] = (tx)(ys * y[:]), the product rounded to f64 first (ys = 1: a plain convert) */
int ssp_mx_copy(ssp_ctx* ctx, void* x, ssp_dtype tx, const void* y, ssp_dtype ty, double ys, size_t n);
/* xx[v][:] = (double)(float)(xs[v] * xx[v][:]) for m f64 vectors, in place and in one launch per 16 vectors:
 * each element becomes the value ssp_mx_copy (F32 <- F64, ys = xs[v]) would store, widened again, so that a
 * later narrowing copy of the vector is exact (the refined f32 Q space of itsolv_hbm.h quantises a new
 * parameter vector BEFORE its action is computed).  xs may be null (all 1); a deferred scale costs no pass
 * of its own.  The same kernel, and the same bits, at every length (exact_max is not looked at); n = 0 and
 * m = 0 return at once.  Ledger name quantise_f32, 16 bytes per element and vector. */
int ssp_quantise_f32(ssp_ctx* ctx, double* const* xx, const double* xs, int m, size_t n);
/* y[:] = (ty)fma(alpha, x[:], y[:]) */
int ssp_mx_axpy(ssp_ctx* ctx, double alpha, const void* x, ssp_dtype tx, void* y, ssp_dtype ty, size_t n);
int ssp_mx_dot(ssp_ctx* ctx, const void* x, ssp_dtype tx, const void* y, ssp_dtype ty, size_t n, double* out);
/* out (m x k, row-major) = <xs[i] xx[i], ys[j] yy[j]> summed over ranks; xs / ys may be null (all 1) */
int ssp_mx_gemm_inner(ssp_ctx* ctx, const void* const* xx, ssp_dtype tx, const double* xs, int m,
                      const void* const* yy, ssp_dtype ty, const double* ys, int k, size_t n, double* out);
/* yy[j] (+)= sum_i alphas[i*m + j] (xs[i] xx[i]); set != 0: the destinations are written, not read
 * (ssp_gemm_outer_set).  No destination may alias a source. */
int ssp_mx_gemm_outer(ssp_ctx* ctx, const double* alphas, const void* const* xx, ssp_dtype tx, const double* xs, int k,
                      void* const* yy, ssp_dtype ty, int m, size_t n, int set);
/* Residuals against right-hand sides, and their norms, in one pass (LinearEquationsDavidson's
 * construct_residual + update_errors, reference LinearEquationsDavidson.h:175-186 and
 * IterativeSolverTemplate.h:95-102; the linear-equations twin of ssp_axpy_pairs_norm):
 *   yy[j][:] = s[j] * (ys[j] * yy[j][:] - (double)bb[j][:]),  out[j] = <yy[j], yy[j]> summed over ranks
 * bb is stored as tb (SSP_F32: the stored right-hand sides of an f32 Q space; SSP_F64: the f64 twins of its
 * refined mode), yy is f64.  ys is the pending scale of yy, applied as yy is loaded (the one rounding an eager
 * ssp_scal stores); it may be null (all 1).  The subtraction is rounded once and the product with s once, with
 * no contraction, so yy is bit-identical to ssp_scal(ys[j]) (where ys[j] != 1), ssp_mx_axpy(-1, bb[j], yy[j])
 * and ssp_scal(s[j]) on the same context -- three launches per vector and a dot, 44 or 48 bytes per element
 * where this pass moves 20 or 24.
 *   - One launch serves m <= 16; more vectors take that unfused sequence and one ssp_dot each.
 *   - The norms are fixed-order sums (per-workgroup partials on a fixed grid, folded by the last workgroup):
 *     repeated calls give the same bits.  On vectors of at most exact_max elements they are the reference's
 *     sequential dots of the unfused sequence, in one reduction.
 *   - With a communicator attached the buffer summed over ranks has length m whatever n is (m <= 16); n = 0
 *     writes zeros; m = 0 returns at once.  Pending zero fills are stored first.
 *   - Every pointer 16-byte aligned and non-null (n > 0); no yy[j] may be a bb[i] or another yy[i].
 * Ledger name rhs_residual_norms, bytes n m (16 + 4 or 8). */
int ssp_mx_rhs_residual_norms(ssp_ctx* ctx, const void* const* bb, ssp_dtype tb, const double* s, double* const* yy,
                              const double* ys, int m, size_t n, double* out);

/* ---- fused solver passes over an f32 Q space beside f64 R vectors (itsolv_hbm/hbm_handlers_f32.h):
 *      the mixed-precision rule above, applied per column / per source.
 *
 * out (m x k, row-major) = <xs[i] xx[i], ys[j] yy[j]> summed over ranks.  Rows are f64; column j is
 * stored as ty[j] (SSP_F64 or SSP_F32), in any order.  xs / ys may be null (all 1).
 *   - One launch per tile of 16 rows x 64 column slots reads its rows once for the columns of both types.
 *     The columns are ordered f64 first and each type padded to whole groups of 4 (csrc/mx_cols_plan.h);
 *     a tile that holds f32 columns only runs on ssp_mx_gemm_inner's kernel.  The result comes back in
 *     the caller's column order.
 *   - On vectors of at most exact_max elements the f32 columns are widened into scratch and every entry
 *     is ssp_gemm_inner_scaled's, bit for bit; else every entry is a fixed-order sum (repeated calls give
 *     the same bits).
 *   - With a communicator attached the buffer summed over ranks is laid out by (m, k, ty[]) alone: the
 *     m x slots layout on the bandwidth path, on the exact path and for an empty shard (n = 0: zeros).
 *   - All-f64 columns forward to ssp_gemm_inner_scaled, all-f32 columns to ssp_mx_gemm_inner (their
 *     own m x k layouts, again whatever n is); m = 0 and k = 0 return at once.
 * Ledger name gemm_inner_cols, bytes n (8 m + the sum of the columns' element sizes). */
int ssp_q32_gemm_inner_cols(ssp_ctx* ctx, const double* const* xx, const double* xs, int m, const void* const* yy,
                            const ssp_dtype* ty, const double* ys, int k, size_t n, double* out);
/* ssp_construct_solution / ssp_block_update with the dense sources stored in f32 (no source scales: an
 * f32 vector carries none); destinations f64.  Bit-identical to the f64 entry point on widened copies of
 * the sources, at the indices the P vectors touch too (P terms first, then the dense sources in order).
 * Ledger: the dense pass counts as gemm_outer_f32 (4 bytes per source element), the fix-up under the f64
 * entry points' names. */
int ssp_q32_construct_solution(ssp_ctx* ctx, const double* palphas, const size_t* ptr, const size_t* idx,
                               const double* val, int kp, const double* alphas, const float* const* xx, int k,
                               double* const* yy, int m, size_t n, size_t offset);
int ssp_q32_block_update(ssp_ctx* ctx, const double* palphas, const size_t* ptr, const size_t* idx, const double* val,
                         int kp, const double* alphas, const float* const* xx, int k, double* const* yy,
                         const double* ys, int m, size_t n, size_t offset);
/* New f32 vectors as combinations of existing ones, with their f64 twins (the consistent D space of the
 * refined f32 Q space, itsolv_hbm/solvers.h set_refine_dspace):
 *   yy[j][:] = (float)(sum_i alphas[i*m + j] xx[i][:])   the f64 sum of the sources in order, rounded once
 *   ww[j][:] = (double)yy[j][:]                            the stored value, widened
 * in one pass that reads the k sources once and reads neither destination set.  Both outputs are bit-identical
 * to ssp_mx_gemm_outer(F32 -> F32, set = 1) followed by ssp_mx_copy(ww[j], SSP_F64, yy[j], SSP_F32, 1.0), at
 * every length and in exact mode (on vectors of at most exact_max elements: the exact path of
 * ssp_mx_gemm_outer, then the widening copies); with more than 64 sources the launches chain as
 * ssp_mx_gemm_outer's do and the last one writes the twins.  Pending zero fills of the destinations are
 * dropped, those of the sources stored.  No destination may alias a source or another destination; k = 0
 * writes zeros; m = 0 and n = 0 return at once.  Ledger name combine_widen_f32, bytes n (4 k + 12 m). */
int ssp_q32_combine_widen(ssp_ctx* ctx, const double* alphas, const float* const* xx, int k, float* const* yy,
                          double* const* ww, int m, size_t n);
/* A DIIS history stored as differences (itsolv_hbm/diis_differences.h): the newest point of each of m series
 * (the parameters and the residuals) is kept in f64 (the anchor aa[j]), every older point as the f32 difference
 * between it and its successor.  A new point vv[j] is taken in by one pass:
 *   dd[j][:] = (float)(vv[j][:] - aa[j][:])   subtracted in f64 (one rounding), narrowed to nearest-even
 *   aa[j][:] = vv[j][:]
 * 28 bytes per element and vector, where ssp_copy to scratch, ssp_axpy(-1), ssp_mx_copy (F32 <- F64) and
 * ssp_copy to the anchor move 68; bit-identical to that sequence at every length and exact_max (each element
 * is one subtraction and one narrowing in either arithmetic).  dd null: aa[j] = vv[j] only (the first point).
 *   - Pending zero fills of vv and aa are stored, those of dd dropped.  Pointers 16-byte aligned; no aa[j] or
 *     dd[j] may be a vv[l], another aa[l] or dd[l] (SSP_ERR_ARG); m = 0 and n = 0 return at once.  One launch
 *     per 16 vectors.  No reduction: nothing is exchanged between ranks.
 * Ledger name store_differences_f32, bytes 28 n m. */
int ssp_q32_store_differences(ssp_ctx* ctx, const double* const* vv, double* const* aa, float* const* dd, int m,
                              size_t n);
/* Combinations of such series, m panels that share one coefficient vector (the parameter and the residual
 * construction of a DIIS step in one launch; m = 1: the parameters alone):
 *   yy[j][:] = aa[j][:] - sum_i gammas[i] (double)dd[j*k + i][:]     j < m, i < k
 * as y = a, then y = fma(-gammas[i], d_i, y) for i = 0..k-1: bit-identical to ssp_copy(yy[j], aa[j]) followed
 * by ssp_mx_gemm_outer(alphas = -gammas, dd + j k, F32 -> yy[j], F64, set = 0), on vectors of at most exact_max
 * elements too (there the pass is that sequence, on the exact path).  The destinations are written, not read:
 * n m (16 + 4 k) bytes, where the sequence moves n m (40 + 4 k).  k = 0 copies the anchors.
 *   - Two panels per launch, 64 differences per launch (more chain: each later launch goes on from what the one
 *     before stored, the same fma chain).  Pending zero fills of aa and dd are stored, those of yy dropped.
 *     Pointers 16-byte aligned; no yy[j] may be an aa[l], a dd[i] or another yy[l] (SSP_ERR_ARG); m = 0 and
 *     n = 0 return at once.  No reduction: nothing is exchanged between ranks.
 * Ledger name anchor_combine_f32, bytes n m (16 + 4 k). */
int ssp_q32_anchor_combine(ssp_ctx* ctx, const double* gammas, const double* const* aa, const float* const* dd, int k,
                           double* const* yy, int m, size_t n);

/* ---- selection: reference util/select.h:28-55, util/select_max_dot.h:166-190,
 *      DistrArray.cpp:170-276.  Local shard [offset, offset+n) of a global array.  Returns up
 *      to nsel (global index, value) pairs in ASCENDING INDEX order (std::map order), chosen
 *      over all ranks with the reference's tie rule (larger index wins a tie). ----------- */
int ssp_select(ssp_ctx* ctx, const double* x, size_t n, size_t offset, size_t nsel, int max, int ignore_sign,
               size_t* idx_out, double* val_out, size_t* nout);
/* Merge of per-rank selections (host only, no context): rank r's count[r] <= stride results are
 * idx/val[r*stride ...] as ssp_select returns them (val = x, |x| or |x*y|).  Keeps the nsel
 * largest (v', index) pairs, v' = max ? val : -val, ties to the larger index, and returns them
 * ordered by index -- the reference heap's result (util/select.h:28-55).  ssp_select and
 * ssp_select_max_dot (max = 1) merge their all-gathered candidates with this function. */
int ssp_select_merge(int nranks, const size_t* counts, size_t stride, const size_t* idx, const double* val,
                     size_t nsel, int max, size_t* idx_out, double* val_out, size_t* nout);
int ssp_select_max_dot(ssp_ctx* ctx, const double* x, const double* y, size_t n, size_t offset, size_t nsel,
                       size_t* idx_out, double* val_out, size_t* nout);

/* ---- dense x sparse (R x P): P = std::map<size_t,double>, passed as sorted global indices.
 *      reference ArrayHandlerIterableSparse.h:35-58, util/gemm.h:207-253,
 *      DistrArray.cpp:419-465.  Entries outside [offset, offset+n) are ignored. ---------- */
/* x = 0 then x[idx-offset] = val */
int ssp_sparse_copy(ssp_ctx* ctx, double* x, size_t n, size_t offset, const size_t* idx, const double* val,
                    size_t nnz);
/* x[idx-offset] += alpha * val */
int ssp_sparse_axpy(ssp_ctx* ctx, double alpha, const size_t* idx, const double* val, size_t nnz, double* x,
                    size_t n, size_t offset);
/* xx[k][idx-offset] += val over the entries [ptr[k], ptr[k+1]) of each of nvec sparse vectors (one
 * ssp_sparse_axpy(1.0) per vector, in one launch for up to 16 vectors and 256 local entries). */
int ssp_sparse_axpy_batch(ssp_ctx* ctx, int nvec, const size_t* ptr, const size_t* idx, const double* val,
                          double* const* xx, size_t n, size_t offset);
/* *out = sum_ranks sum_e x[idx_e-offset] * val_e */
int ssp_sparse_dot(ssp_ctx* ctx, const double* x, size_t n, size_t offset, const size_t* idx, const double* val,
                   size_t nnz, double* out);
/* out (m x k) = <xx[i], p_j>; p_j = entries [ptr[j], ptr[j+1]) of (idx, val). */
int ssp_gemm_inner_sparse(ssp_ctx* ctx, const double* const* xx, int m, size_t n, size_t offset, const size_t* ptr,
                          const size_t* idx, const double* val, int k, double* out);
/* yy[j] += sum_i alphas[i*m + j] * p_i; p_i = entries [ptr[i], ptr[i+1]). */
int ssp_gemm_outer_sparse(ssp_ctx* ctx, const double* alphas, const size_t* ptr, const size_t* idx,
                          const double* val, int k, double* const* yy, int m, size_t n, size_t offset);

/* construct_solution (reference IterativeSolverTemplate.h:33-65: fill(0), then gemm_outer over the
 * P, Q and D spaces) in one pass that does not read the destinations:
 *   yy[j] = sum_i palphas[i*m + j] p_i  +  sum_s alphas[s*m + j] xx[s]
 * with P = CSR (ptr, idx, val) of kp sparse vectors (global indices), bit-identical to
 * ssp_fill(0) + ssp_gemm_outer_sparse + ssp_gemm_outer (Q and D sources concatenated). */
int ssp_construct_solution(ssp_ctx* ctx, const double* palphas, const size_t* ptr, const size_t* idx,
                           const double* val, int kp, const double* alphas, const double* const* xx, int k,
                           double* const* yy, int m, size_t n, size_t offset);

/* ---- synthetic problem (harness only; not a reference operation) ----------------------------
 * H = diag(d) + rho * sum_{l<rank} u_l u_l^T, g = global index, u_0 = 1 and for l > 0
 * u_l(g) = +/-1 from a splitmix64 hash of (seed, l, g).  The rank-one (rank=1) case is the
 * matrix of reference test/itsolv/test_rayleigh_quotient.cpp:37-42.  yy[v] = H xx[v].
 * Diagonal families (itsolv_hbm/problems.h SyntheticSpec):
 *   SSPX_DIAG_LINEAR   d_g = 1 + g; sspx_synth_diagonal reports H_gg = 1 + g + rank*rho
 *   SSPX_DIAG_BOUNDED  d_g = 1 + 2 frac(g phi1); sspx_synth_diagonal reports the approximate
 *                      diagonal d_g (1 + alpha (2 frac(g phi2) - 1)) (C5's DIIS preconditioner) */
#define SSPX_DIAG_LINEAR 0
#define SSPX_DIAG_BOUNDED 1
typedef struct {
  double rho;
  int rank;                /* 1..16 */
  unsigned long long seed;
  int diag_kind;           /* SSPX_DIAG_* */
  double alpha;            /* SSPX_DIAG_BOUNDED: preconditioner mismatch */
  double target;           /* NonLinearEquations residual r = H (x - target 1); 0 is read as 1 (the
                              reference test's x = 1) */
} sspx_synth;
int sspx_synth_action(ssp_ctx* ctx, const sspx_synth* spec, const double* const* xx, double* const* yy, int nvec,
                      size_t n, size_t offset);
/* yy[v] = H (xs[v] xx[v]): the action on deferred-scaled parameters (xs may be null) */
int sspx_synth_action_scaled(ssp_ctx* ctx, const sspx_synth* spec, const double* const* xx, const double* xs,
                             double* const* yy, int nvec, size_t n, size_t offset);
/* yy[v] += rho * sum_l w[v*rank + l] u_l */
int sspx_synth_add_lowrank(ssp_ctx* ctx, const sspx_synth* spec, double* const* yy, int nvec, size_t n,
                           size_t offset, const double* w);
int sspx_synth_diagonal(ssp_ctx* ctx, const sspx_synth* spec, double* d, size_t n, size_t offset);
/* The SSPX_DIAG_LINEAR forms of the three calls above. */
int sspx_synthetic_action(ssp_ctx* ctx, const double* const* xx, double* const* yy, int nvec, size_t n,
                          size_t offset, double rho, int rank, unsigned long long seed);
/* yy[v] += rho * sum_l w[v*rank + l] u_l  (the low-rank part of H applied to P-space vectors) */
int sspx_synthetic_add_lowrank(ssp_ctx* ctx, double* const* yy, int nvec, size_t n, size_t offset, double rho,
                               int rank, unsigned long long seed, const double* w);
/* d[g] = H_gg = 1 + g + rank*rho */
int sspx_synthetic_diagonal(ssp_ctx* ctx, double* d, size_t n, size_t offset, double rho, int rank);
/* x[g] = uniform [-1,1) from splitmix64(seed, vec, g): G-independent benchmark data. */
int sspx_fill_random(ssp_ctx* ctx, double* x, size_t n, size_t offset, unsigned long long seed,
                     unsigned long long vec);
/* Test harness: occupies the context's stream for `ms` milliseconds (one workgroup spinning on the
 * device clock; always ends), to exercise the communication deadline. */
int sspx_debug_stall(ssp_ctx* ctx, double ms);
/* y = A x for a dense row-major n_global x n_global matrix A in device memory, local rows
 * [offset, offset+n) of y; x must be the full (gathered) vector.  Used for small fixtures. */
int sspx_dense_action(ssp_ctx* ctx, const double* a, size_t n_global, const double* const* xx, double* const* yy,
                      int nvec, size_t n, size_t offset);

#ifdef __cplusplus
}
#endif
#endif /* SUBSPACE_HIP_H */
