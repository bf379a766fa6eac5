/*
 * itsolv_hbm.h — C ABI of libitsolv_hbm.so: the host C++ solvers (LinearEigensystemDavidson,
 * NonLinearEquationsDIIS; restated from the reference's itsolv headers) running over the HBM handlers of
 * libsubspace_hip.so.  These entry points drive a complete solve on a problem whose action is
 * computed on the device, and report what the reference's tests check: eigenvalues, errors,
 * statistics().iterations, and recomputed residual norms.
 *
 * The context is a libsubspace_hip.so ssp_ctx (with an RCCL communicator attached for more than
 * one rank); every rank calls the same entry point with the same arguments (SPMD, as the
 * reference's MPI build requires).  The oracle (oracle/itsolv_oracle.cpp) exports the same
 * functions with an `oracle_` prefix and std::vector<double> CPU handlers.
 */
#ifndef ITSOLV_HBM_H
#define ITSOLV_HBM_H
#include <stddef.h>

#include "subspace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ITSOLV_MAX_ROOTS 64
#define ITSOLV_TRACE_ITER 256
#define ITSOLV_TRACE_ROOTS 8

typedef struct {
  int nroots;                  /* n_roots (reference Options::n_roots)                    */
  int nwork;                   /* number of R buffers handed to solve(); 0 -> nroots       */
  int max_iter;                /* reference IterativeSolverTemplate m_max_iter (default 100) */
  int max_size_qspace;         /* reference option max_size_qspace (<= 0: unlimited)       */
  int reset_D;                 /* reference option reset_D (<= 0: never)                   */
  int reset_D_max_Q_size;      /* <= 0: unlimited                                          */
  int max_p;                   /* P-space size limit (0: no P space)                       */
  double p_threshold;          /* P-space selection threshold (<= 0: infinity)             */
  double convergence_threshold;
  int hermitian;
  int generate_initial_guess;  /* 1: initial guess from the n smallest diagonals           */
  int verbosity;               /* 0 none .. 3 detailed                                     */
  double augmented_hessian;    /* LinearEquationsDavidson augmented-Hessian parameter (0: off) */
  int block_gram_schmidt;      /* extension (-1: the vector type's default, 0: the reference's MGS,
                                  1: on): orthogonalise the new
                                  R vectors against P, Q, D with coefficients from the overlaps
                                  already computed for redundancy screening (forward substitution
                                  through the stored S) and one gemm_outer per space; same result
                                  in exact arithmetic, not bit-identical */
} itsolv_options;

typedef struct {
  int converged;
  int iterations;      /* statistics().iterations                                          */
  int r_creations;
  int q_creations;
  int nroots;
  double eigenvalues[ITSOLV_MAX_ROOTS];
  double errors[ITSOLV_MAX_ROOTS];
  double residual_norms[ITSOLV_MAX_ROOTS]; /* |H x - e x| / |x| recomputed from solution() */
  double seconds;      /* wall time of the solve                                            */
  int n_eig_trace;     /* iterations recorded in eig_trace (<= 256)                          */
  double eig_trace[256]; /* lowest eigenvalue after each add_vector                          */
  /* Per-iteration trace (the parity observables of IterativeSolverTemplate.h:322-408), one row
   * per solve() iteration, n_eig_trace rows: eigenvalues (Davidson) and errors of the first
   * trace_roots roots, Q-space size and working-set size after the iteration. */
  int trace_roots;
  int trace_nq[ITSOLV_TRACE_ITER];
  int trace_nwork[ITSOLV_TRACE_ITER];
  double trace_eigenvalues[ITSOLV_TRACE_ITER * ITSOLV_TRACE_ROOTS];
  double trace_errors[ITSOLV_TRACE_ITER * ITSOLV_TRACE_ROOTS];
  /* propose_rspace's screening (extension): new R vectors removed by the redundancy screen and as
   * null after orthogonalisation, in all, and cumulative after each iteration */
  int redundant_params;
  int null_params;
  int trace_screened[ITSOLV_TRACE_ITER];
  /* host time of the subspace algebra (extension, instrumentation): wall seconds, calls and the
   * largest dimension of the eigenproblem / svd_system / solve_DIIS / solve_LinearEquations calls
   * of the solve (itsolv_hbm/dense.h AlgebraClock) */
  double host_algebra_seconds;
  int host_algebra_calls;
  int host_algebra_max_dim;
} itsolv_result;

const char* itsolv_last_error(void);
void itsolv_default_options(itsolv_options* opt);

/* Davidson on H = diag(1+g) + rho * sum_{l<rank} u_l u_l^T (global length n, sharded over the
 * context's ranks).  solutions_out (optional): this rank's shard of each root, nroots x n_local. */
int itsolv_davidson_synthetic(ssp_ctx* ctx, size_t n, double rho, int rank, unsigned long long seed,
                              const itsolv_options* opt, itsolv_result* out, double* solutions_out);

/* Davidson on a dense n x n row-major matrix (small fixtures; single rank). */
int itsolv_davidson_dense(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                          double* solutions_out);

/* DIIS on the residual r(x) = H (x - 1) of the synthetic H (solution x = 1), diagonal
 * preconditioner, x0 = 0 except x0[0] = 1.  x_out (optional): this rank's shard of the solution. */
int itsolv_diis_synthetic(ssp_ctx* ctx, size_t n, double rho, int rank, unsigned long long seed,
                          const itsolv_options* opt, itsolv_result* out, double* x_out);

/* The same two solves on any synthetic family (subspace_hip.h sspx_synth), e.g. BASELINE config
 * C5's well-posed DIIS instance: diag_kind SSPX_DIAG_BOUNDED, rho = 1/n, rank 1, alpha 0.5
 * (itsolv_hbm/problems.h c5_spec). */
int itsolv_davidson_synth(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                          itsolv_result* out, double* solutions_out);
int itsolv_diis_synth(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt, itsolv_result* out,
                      double* x_out);

/* itsolv_davidson_dense / itsolv_davidson_synth with the Q space STORED in f32 (itsolv_hbm/hbm_vec_f32.h,
 * LinearEigensystemDavidson<Vec, VecF32, SparseP> over make_handlers_q32()): R vectors, the subspace
 * matrices and every kernel's arithmetic stay f64; a Q vector is rounded once, to nearest-even, when it
 * is stored.  Half the HBM per Q vector and half the bytes of every pass over the Q space.  Eigenvalues
 * move by at most about 4 eps32 |H| (first-order perturbation of the stored vectors), and the residual
 * the solver estimates from the stored pairs floors near eps32 |a|: with these two entries convergence
 * thresholds down to about 1e-6 |H| are meaningful (below, the solve stalls; use the refined entries).
 * Same arguments and results as the f64 entries. */
int itsolv_davidson_dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                              double* solutions_out);
int itsolv_davidson_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                              itsolv_result* out, double* solutions_out);

/* The same two solves in the REFINED mode of the f32 Q space (itsolv_hbm/solvers.h set_refine), which reaches
 * f64 thresholds (1e-8, 1e-10) with the Q space still in 4 bytes per element:
 *   1. a new parameter vector is rounded to f32-representable values (ssp_quantise_f32) BEFORE its action
 *      is computed, so the stored vector is exact and the action belongs to it;
 *   2. the new rows of the subspace H come from the stored Q parameters and the new f64 actions, not from
 *      the stored f32 actions: S and H are the exact f64 projection onto the span of the stored vectors;
 *   3. only the stored actions then carry error, bounded for root i by
 *      delta_i = 2^-24 sum_j |c_ji| |a_j|.  A root whose residual estimate is <= max(kappa delta_i,
 *      threshold + delta_i) has its residual recomputed from the action of its solution.
 * The price: until that point a root costs nothing extra; from it on, ONE MORE ACTION per such root and
 * iteration (all refined roots of an iteration in one action call; a converged root stays among them, as
 * the solver recomputes every root's residual in every iteration).  The errors reported for converged
 * roots are then true residual norms, not estimates.
 * Scope: hermitian = 1 only; max_size_qspace, reset_D and reset_D_max_Q_size must be unset (a D space holds
 * rounded combinations whose pairs are inconsistent in the way step 1 removes for Q); each is refused with
 * an error that names the option.  refine: NULL for the defaults; kappa <= 0 means the default of 8. */
typedef struct {
  double kappa;
} itsolv_q32_refine;
int itsolv_davidson_dense_q32_refined(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt,
                                      const itsolv_q32_refine* refine, itsolv_result* out, double* solutions_out);
int itsolv_davidson_synth_q32_refined(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                                      const itsolv_q32_refine* refine, itsolv_result* out, double* solutions_out);
/* What the calling thread's last refined solve spent (thread-local, as itsolv_last_error): actions on refined
 * residuals, the iteration (from 1; 0: none) of the first, the largest of the roots' last delta.  Any
 * pointer may be NULL.  Returns 0. */
int itsolv_q32_refine_stats(int* refined_actions, int* first_refined_iteration, double* max_delta);

/* The refined mode UNDER A Q-SPACE LIMIT (itsolv_hbm/solvers.h set_refine_dspace): the two refined solves with
 * max_size_qspace admitted.  Whenever the limit deletes Q vectors the D space is rebuilt consistently:
 *   - the new D parameters are written by one pass over the parameters of the deleted Q vectors and of the old
 *     D space (ssp_q32_combine_widen: each the f64 sum of its sources, rounded once, with the stored value
 *     widened beside it); the stored Q / D actions are not read and nothing is rescaled after the rounding;
 *   - the D actions are TRUE actions of exactly those stored vectors, one action call for all of them;
 *   - the D blocks of S and H come from these in f64, and the bound delta_i gains the D terms
 *     2^-24 sum_d |c_di| |a_d|.
 * The price: nD <= nroots more actions per rebuild.  What a rebuild cannot keep is the part of the solutions
 * that the rounding of the new D parameters removes from the subspace (2^-24 of each element), which later
 * iterations restore at the solver's convergence rate; so a rebuild cuts the Q space up to two working sets
 * BELOW max_size_qspace (never a quarter of it; nothing where the limit is below about 8 nroots) and the next
 * comes two or three iterations later.  Where nothing is cut every iteration rebuilds, and thresholds within a
 * small multiple of 2^-24 |H - lambda| |tail of the solution| are out of reach.
 * Scope: as the refined entries, with max_size_qspace allowed; reset_D and an explicit reset_D_max_Q_size
 * stay refused.  Same arguments as the refined entries. */
int itsolv_davidson_dense_q32_refined_dspace(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt,
                                             const itsolv_q32_refine* refine, itsolv_result* out,
                                             double* solutions_out);
int itsolv_davidson_synth_q32_refined_dspace(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                                             const itsolv_q32_refine* refine, itsolv_result* out,
                                             double* solutions_out);
/* What the calling thread's last such solve spent on its D space: rebuilds, and the actions on them (these
 * are not among itsolv_q32_refine_stats' refined_actions).  Any pointer may be NULL.  Returns 0. */
int itsolv_q32_dspace_stats(int* rebuilds, int* actions);

/* DIIS on r(x) = H (x - 1) for a dense row-major H (reference test_NonLinearEquations.cpp:38-49). */
/* LinearEquationsDavidson (reference itsolv/LinearEquationsDavidson.h): A x_r = b_r for nrhs
 * right-hand sides b (row-major nrhs x n, host), dense row-major A resident in HBM (single rank).
 * x_out (nrhs x n, host) may be NULL. */
int itsolv_linear_equations_dense(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                  const itsolv_options* opt, itsolv_result* out, double* x_out);
/* The same solver at scale: A is the synthetic H of sspx_synth (symmetric positive definite for rho >= 0;
 * action, diagonal and preconditioner on the device, as itsolv_davidson_synth's), sharded over the ranks of
 * ctx in the same way, and the right-hand sides are b_r = sspx_fill_random(seed = rhs_seed, vec = r) at the
 * shard's global offset, r < nrhs <= ITSOLV_MAX_ROOTS.  residual_norms are |A x_r - b_r| / |b_r| recomputed
 * from the action; x_out (nrhs x the local length, host) may be NULL. */
int itsolv_linear_equations_synth(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs, unsigned long long rhs_seed,
                                  const itsolv_options* opt, itsolv_result* out, double* x_out);
/* Linear equations with the Q space stored in f32 (one rank).
 *   *_q32          plain: the right-hand sides are stored rounded with the Q space, so the true residual cannot
 *                  fall below about 2^-24 |b|: meaningful down to thresholds of about 1e-6, as the plain f32
 *                  eigensolver.  Every option of the f64 solver is allowed.
 *   *_q32_refined  the refined mode (itsolv_davidson_*_q32_refined): new parameters quantised before their
 *                  action, H rows from f64 actions, an f64 twin of every right-hand side beside the stored one
 *                  (the subspace rhs rows and the residuals read the twin only), and residuals recomputed from
 *                  the action of the solution where the bound delta_i = 2^-24 sum_j |c_ji| |a_j| / |b_i| no
 *                  longer vouches for the estimate.  It reaches f64 thresholds at one more action per refined
 *                  root and iteration; the reported errors are then true relative residuals.  Scope: hermitian = 1,
 *                  max_size_qspace, reset_D and reset_D_max_Q_size unset, augmented_hessian = 0; anything else
 *                  is an error naming the option.  refine may be NULL (kappa = 8); itsolv_q32_refine_stats
 *                  reports what the solve spent. */
int itsolv_linear_equations_dense_q32(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                      const itsolv_options* opt, itsolv_result* out, double* x_out);
int itsolv_linear_equations_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs,
                                      unsigned long long rhs_seed, const itsolv_options* opt, itsolv_result* out,
                                      double* x_out);
int itsolv_linear_equations_dense_q32_refined(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                              const itsolv_options* opt, const itsolv_q32_refine* refine,
                                              itsolv_result* out, double* x_out);
int itsolv_linear_equations_synth_q32_refined(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs,
                                              unsigned long long rhs_seed, const itsolv_options* opt,
                                              const itsolv_q32_refine* refine, itsolv_result* out, double* x_out);
/* OptimizeBFGS (algorithm 0) or OptimizeSD (1) minimising the Rayleigh quotient x.Hx / x.x of a
 * dense row-major H (HBM, single rank) from x = e_0; eigenvalues[0] = final function value, x_out
 * (n, host) may be NULL. */
int itsolv_optimize_dense(ssp_ctx* ctx, const double* h, size_t n, int algorithm, const itsolv_options* opt,
                          itsolv_result* out, double* x_out);
int itsolv_diis_dense(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                      double* x_out);
/* DIIS with its history in f32 (itsolv_hbm/diis_differences.h: NonLinearEquationsDIISDifferences<Vec, VecF32,
 * SparseP> over make_handlers_q32()), the problems, options and result of itsolv_diis_synth / itsolv_diis_dense.
 * The history is not k rounded (parameter, residual) pairs -- rounding every iterate leaves the residual stuck near
 * 2^-24 |J| |x*| -- but two f64 anchors (the newest pair) and k - 1 pairs of f32 differences between successive
 * iterates, each rounded once: what the rounding loses shrinks with the error, so f64 thresholds are reached in
 * the iterations of the f64 solve, with no extra residual evaluation and no mode flag.  A history of k pairs
 * takes (k - 1) 8 n + 16 n bytes where the f64 solve takes 16 k n.  A new pair is taken in by one
 * ssp_q32_store_differences, the new row of the DIIS matrix is one ssp_q32_gemm_inner_cols (r_0 against itself
 * and the k - 1 residual differences), and both constructions of a step are one ssp_q32_anchor_combine.
 * max_size_qspace and the svd pruning act as in the f64 solve.  Refused, the message naming it: max_p > 0 (a P
 * space), and a context with more than one rank. */
int itsolv_diis_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt, itsolv_result* out,
                          double* x_out);
int itsolv_diis_dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                          double* x_out);
/* What the last itsolv_diis_*_q32 solve of this thread held when it ended: the points of its history, the pairs
 * of f32 differences among them (points - 1), and the bytes of the context's arena in use by the history (the
 * anchors and the differences; from ssp_memory_stats around the solver's life).  Any pointer may be NULL.
 * Returns 0. */
int itsolv_q32_diis_stats(int* points, int* pairs, size_t* history_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ITSOLV_HBM_H */
