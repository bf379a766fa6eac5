/*
 * iterative_solver_c.h — the reference's reverse-communication C API (what Molpro's Fortran and
 * the Python extension bind) on the MI355X back end, exported by libitsolv_hbm.so.
 *
 * Every declaration below has the name, argument list and meaning of the reference's
 * src/molpro/linalg/IterativeSolverC.h:6-73 (implementation IterativeSolverCMPI.cpp:158-534):
 *  - R vectors are the caller's host arrays, `buffer_size` vectors of length `dimension` stored
 *    one after the other; this rank works on [range_begin, range_end) of each (the reference's
 *    make_distribution_spread_remainder layout), returned by the *Initialize calls;
 *  - with `sync` != 0 the updated vectors are gathered in full on every rank;
 *  - Q (and D) vectors live in HBM instead of DistrArrayFile: every subspace operation runs on the
 *    device, and R crosses PCIe once per call in each direction;
 *  - the solver instances form a stack; only the top one is active (as in the reference).
 *
 * Differences:
 *  - `fcomm` (a Fortran MPI communicator, reference IterativeSolverCMPI.cpp:169 MPI_Comm_f2c(fcomm))
 *    is bridged at run time to the MPI library the calling process has loaded and initialised
 *    (libitsolv_hbm.so does not link MPI; iterative-solver_amd/host/mpi_bridge.h).  With more than
 *    one rank the instance's vectors are sharded over the communicator's ranks exactly as the
 *    reference distributes them (make_distribution_spread_remainder, :79-105), each rank's shard in
 *    the HBM of the device matching its place among the communicator's ranks on its node, and the
 *    reductions / sync gathers run over the transport ITSOLV_HBM_COMM names: "mpi" (default:
 *    MPI_Allreduce / MPI_Allgather on the communicator, the reference's own collectives), "p2p"
 *    (peer-memory device exchange, one node) or "rccl" (RCCL over xGMI, one rank per device).
 *    Precedence: a context set by IterativeSolverHbmSetContext; else fcomm when MPI is initialised in
 *    the process and fcomm names a communicator; else a single-rank context on the device of the
 *    node-local rank the launcher exports (LOCAL_RANK, OMPI_COMM_WORLD_LOCAL_RANK, MPI_LOCALRANKID or
 *    SLURM_LOCALID, first one set, modulo the visible device count; device 0 without any of them).
 *  - Supported algorithms: LinearEigensystem and LinearEquations "Davidson" (or ""),
 *    NonLinearEquations "DIIS" (or ""), Optimize "BFGS" (or "") and "SD"; `minimize` is ignored,
 *    as in the reference (IterativeSolverCMPI.cpp:250-268).
 *  - Davidson instances (LinearEigensystem, LinearEquations) orthogonalise new R vectors by block
 *    Gram-Schmidt (coefficients by forward substitution through the stored overlaps, one gemm_outer
 *    per space): the same projection as the reference's sequential MGS in exact
 *    arithmetic, not bit-identical.  "BLOCK_GRAM_SCHMIDT=false" in the options string restores
 *    the reference's MGS.
 *  - IterativeSolverAddVector on a non-linear solver (DIIS) passes the vector through the solver's
 *    own add_vector (residual norm, convergence flag, least-important-vector deletion), as the
 *    reference's solve() driver does; the reference's C layer reaches the generic vector-list
 *    overload, which skips that logic.
 *  - Errors are thrown as C++ exceptions, exactly as the reference's extern "C" functions do,
 *    unless IterativeSolverHbmSetThrow(0) selects recorded errors (IterativeSolverHbmLastError).
 */
#ifndef ITERATIVE_SOLVER_C_H
#define ITERATIVE_SOLVER_C_H
#include <stddef.h>
#include <stdint.h>

#include "subspace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

void IterativeSolverLinearEigensystemInitialize(size_t nQ, size_t nroot, size_t* range_begin, size_t* range_end,
                                                double thresh, double thresh_value, int hermitian, int verbosity,
                                                const char* fname, int64_t fcomm, const char* algorithm,
                                                const char* options);
void IterativeSolverLinearEquationsInitialize(size_t n, size_t nroot, size_t* range_begin, size_t* range_end,
                                              const double* rhs, double aughes, double thresh, double thresh_value,
                                              int hermitian, int verbosity, const char* fname, int64_t fcomm,
                                              const char* algorithm, const char* options);
void IterativeSolverNonLinearEquationsInitialize(size_t n, size_t* range_begin, size_t* range_end, double thresh,
                                                 int verbosity, const char* fname, int64_t fcomm,
                                                 const char* algorithm, const char* options);
void IterativeSolverOptimizeInitialize(size_t n, size_t* range_begin, size_t* range_end, double thresh,
                                       double thresh_value, int verbosity, int minimize, const char* fname,
                                       int64_t fcomm, const char* algorithm, const char* options);
void IterativeSolverFinalize(void);
size_t IterativeSolverAddVector(size_t buffer_size, double* parameters, double* action, int sync);
void IterativeSolverSolution(int nroot, int* roots, double* parameters, double* action, int sync);
size_t IterativeSolverAddValue(double value, double* parameters, double* action, int sync);
size_t IterativeSolverEndIteration(size_t buffer_size, double* solution, double* residual, int sync);
int IterativeSolverEndIterationNeeded(void);
size_t IterativeSolverAddP(size_t buffer_size, size_t nP, const size_t* offsets, const size_t* indices,
                           const double* coefficients, const double* pp, double* parameters, double* action, int sync,
                           void (*func)(const double*, double*, const size_t, const size_t*));
void IterativeSolverErrors(double* errors);
void IterativeSolverEigenvalues(double* eigenvalues);
void IterativeSolverWorkingSetEigenvalues(double* eigenvalues);
size_t IterativeSolverSuggestP(const double* solution, const double* residual, size_t maximumNumber, double threshold,
                               size_t* indices);
void IterativeSolverPrintStatistics(void);
int IterativeSolverNonLinear(void);
int IterativeSolverHasValues(void);
int IterativeSolverHasEigenvalues(void);
void IterativeSolverSetDiagonals(const double* diagonals);
void IterativeSolverDiagonals(double* diagonals);
double IterativeSolverValue(void);
int IterativeSolverVerbosity(void);
int IterativeSolverMaxIter(void);
void IterativeSolverSetMaxIter(int max_iter);
int64_t mpicomm_self(void);
int64_t mpicomm_global(void);
int64_t IterativeSolver_mpicomm_global(void);
int64_t IterativeSolver_mpicomm_self(void);
/* IterativeSolverCMPI.cpp:481-534 through the caller's MPI library when it has one: the Fortran
 * handles of MPI_COMM_WORLD / MPI_COMM_SELF (0 without MPI), the world's size and rank (without MPI:
 * those of the context set by IterativeSolverHbmSetContext, else 1 and 0), MPI_Init when MPI is
 * loaded but not initialised, and MPI_Finalize of an MPI initialised that way (0 otherwise).  The
 * _mpi_size_/_mpi_rank_ spellings are the names the reference's Fortran module binds
 * (IterativeSolverF.F90:50-57). */
int64_t IterativeSolver_mpisize_global(void);
int64_t IterativeSolver_mpirank_global(void);
int64_t IterativeSolver_mpi_size_global(void);
int64_t IterativeSolver_mpi_rank_global(void);
int IterativeSolver_mpi_init(void);
int IterativeSolver_mpi_finalize(void);

/* ---- extension: device / communicator selection ----------------------------------------- */
/* Use `ctx` (not owned) for the instances initialised after this call; NULL restores the
 * default (a private single-rank context on the node-local rank's device, see above).  Returns 0. */
int IterativeSolverHbmSetContext(ssp_ctx* ctx);
/* enable = 0: errors are recorded (IterativeSolverHbmLastError, cleared by every call) instead of
 * thrown, and the failing call returns 0 -- for callers that cannot unwind C++ exceptions
 * (ctypes, Fortran).  Default 1 (throw, as the reference does).  Returns 0. */
int IterativeSolverHbmSetThrow(int enable);
/* Statistics of the top instance: iterations, R and Q creations (for tests and reports). */
int IterativeSolverHbmStatistics(int* iterations, int* r_creations, int* q_creations);
const char* IterativeSolverHbmLastError(void);
/* Id (> 0) of the top instance, 0 when there is none.  Ids are unique within the process. */
uint64_t IterativeSolverHbmInstanceId(void);
/* Removes the instance with this id wherever it sits in the stack (a binding whose solver object
 * is destroyed after a newer one was created must not pop the newer one, which
 * IterativeSolverFinalize would).  Returns 0, or 1 when no instance has that id. */
int IterativeSolverHbmFinalizeInstance(uint64_t id);
/* 1 when the process has an MPI library loaded and initialised (MPI_Init done, MPI_Finalize not),
 * i.e. when the *Initialize calls bridge `fcomm`; 0 otherwise. */
int IterativeSolverHbmMpiActive(void);
/* Attaches `ctx` to the ranks of the Fortran MPI communicator `fcomm` over `transport` ("mpi", "p2p",
 * "rccl"; NULL or "" -> ITSOLV_HBM_COMM, else "mpi") -- the attach the *Initialize calls perform for
 * their own contexts, for callers that drive ssp contexts directly.  Collective over fcomm.  Returns
 * 0, or 1 (IterativeSolverHbmLastError) in no-throw mode. */
int IterativeSolverHbmMpiAttach(ssp_ctx* ctx, int64_t fcomm, const char* transport);
/* Number of roots of the top instance (0 when there is none): the length of the arrays
 * IterativeSolverErrors / IterativeSolverEigenvalues fill (used by the Fortran module). */
size_t IterativeSolverHbmNRoots(void);

/* ---- extension: R vectors in device memory ------------------------------------------------
 * The device forms of the calls that stage R.  Each does exactly what its host twin does between
 * copying the caller's arrays in and copying them out again -- the same solver call on the same
 * staging vectors, including the non-linear branch of IterativeSolverAddVector -- with the two
 * PCIe copies replaced by one device-to-device pass each (ssp_rows_import / ssp_rows_export,
 * include/subspace_hip.h; a vector's pending normalisation scale is applied by the export itself).
 *  - The pointers are DEVICE memory on the instance's device and hold THIS RANK'S SHARD only: row k
 *    is [p + k*ld, p + k*ld + local), local = range_end - range_begin as returned by *Initialize,
 *    ld >= local.  Any double* base and any ld are accepted (rows at 8 mod 16 move with 8-byte
 *    accesses); an even ld over a 16-byte aligned base is the fast path.  The calls without an ld
 *    (AddValue, SetDiagonals, Diagonals) move one row.  The block must not overlap the library's own
 *    vectors.
 *  - There is no `sync` argument: gathering a working set into global arrays on every rank is a notion
 *    of host arrays.
 *  - Stream contract: the work is enqueued on the instance's context stream (ssp_ctx_stream).  Whatever
 *    produces the inputs must be ordered on that stream, or finished, before the call; on return the
 *    outputs are ordered on that stream (a consumer on it needs no synchronisation, any other consumer
 *    ssp_synchronize).  The scalar results (return values, Errors, Eigenvalues) are host values as before.
 *  - Host and device forms may be mixed call by call on one instance: both only stage.  This is how a P
 *    space enters -- IterativeSolverAddP stays host-only, device calls follow it.
 *  - Out of scope: a device-side apply_on_p callback, and the Fortran module (it binds the host forms).
 *  - Errors as for the host forms; a library vector layer without the row-block entry points (the CPU
 *    emulation used by the tests) moves 16-byte aligned rows one by one and refuses a misaligned row
 *    before anything has been staged. */
size_t IterativeSolverHbmAddVectorDevice(size_t buffer_size, double* parameters, double* action, size_t ld);
void IterativeSolverHbmSolutionDevice(int nroot, int* roots, double* parameters, double* action, size_t ld);
size_t IterativeSolverHbmAddValueDevice(double value, double* parameters, double* action);
size_t IterativeSolverHbmEndIterationDevice(size_t buffer_size, double* solution, double* residual, size_t ld);
void IterativeSolverHbmSetDiagonalsDevice(const double* diagonals);
void IterativeSolverHbmDiagonalsDevice(double* diagonals);

/* ---- extension: the Q space in f32, and refined residuals -----------------------------------
 * Two options of IterativeSolverLinearEigensystemInitialize's `options` string, for the one-rank "Davidson"
 * (an instance that names neither is what it always was):
 *   Q_STORAGE=f32   (default f64) the Q vectors are stored in 4 bytes per element: half the HBM and half the
 *                   bytes of every pass over them; all arithmetic stays FP64 (include/itsolv_hbm.h *_q32).
 *                   Thresholds are meaningful down to about 1e-6 |H|; below that the solve stalls.
 *   Q_REFINE=1      with optional Q_REFINE_KAPPA=<kappa> (default 8): the refined mode of
 *                   itsolv_hbm/solvers.h set_refine.  A root whose residual estimate the rounding of the stored
 *                   actions no longer vouches for gets its residual from the action of its own solution, which
 *                   the caller supplies through IterativeSolverHbmSetRefineAction; with it an f32 Q space
 *                   reaches f64 thresholds (1e-10).  Allowed with Q_STORAGE=f64 too: nothing is rounded there
 *                   (delta = 0), and the only effect is that a root is declared converged on the residual of
 *                   its solution's own action.
 *   Q_REFINE_DSPACE=1  (needs Q_REFINE=1; refused by name without it) the refined mode under a Q-space limit:
 *                   MAX_SIZE_QSPACE is then allowed, and whenever the limit deletes Q vectors the D space is
 *                   rebuilt consistently (itsolv_hbm/solvers.h set_refine_dspace): new D parameters from the
 *                   stored parameters alone, rounded once, and TRUE actions of exactly those vectors, which the
 *                   refine action supplies -- nD <= nroot more actions per rebuild, in one call.  The rebuild
 *                   happens inside IterativeSolverEndIteration and its device form, whose two arrays are free as
 *                   scratch once imported: the refine action is called there with rows [0, nD) of them, under
 *                   the contract below.  RESET_D and RESET_D_MAX_Q_SIZE stay refused.
 *                   A rebuild cuts the Q space somewhat below the limit, so that rebuilds (each rounds the D
 *                   parameters once more) do not come in every iteration: by two working sets where that is
 *                   under a quarter of the limit, else by one, else not at all.  Q_REFINE_DSPACE_SLACK=<n>
 *                   (needs Q_REFINE_DSPACE=1; n >= 0) sets the number of vectors instead; 0 is the schedule of
 *                   the plain solver, a rebuild in every iteration once the Q space is full.  With a limit under
 *                   about 8 nroot the mode may stall short of an f64 threshold (near 1e-10 |H|).
 * Refused, each with an error that names the option (recorded, not thrown, after IterativeSolverHbmSetThrow(0)):
 * an unknown Q_STORAGE value; either option on Optimize or RSPT, Q_REFINE on NonLinearEquations (Q_STORAGE=f32
 * there: below); either option on an instance with more than one rank; Q_REFINE with hermitian = 0, MAX_SIZE_QSPACE, RESET_D or
 * RESET_D_MAX_Q_SIZE (the refined mode has no D space); Q_STORAGE=f32 over a vector library without the
 * mixed-precision ABI.  Out of scope: multi-rank f32 instances, a D space or a Q-space limit in refined mode
 * without Q_REFINE_DSPACE=1, the D-space reset in refined mode,
 * f32 Q for the optimisers (BFGS, SD), a Fortran binding of the refine callback (the Fortran module passes
 * `options` through, so the plain Q_STORAGE=f32 works from Fortran), a device-side apply_on_p.
 *
 * Non-linear equations.  IterativeSolverNonLinearEquationsInitialize accepts Q_STORAGE=f32 (one rank, "DIIS"): the
 * instance's solver is NonLinearEquationsDIISDifferences (itsolv_hbm/diis_differences.h), whose history is two f64
 * anchors (the newest parameters and residual) and, for every older point, an f32 pair of differences between
 * successive iterates -- (k - 1) 8 n + 16 n bytes for k points where the f64 instance holds 16 k n.  The
 * differences shrink with the error, so f64 thresholds are reached in the f64 instance's iterations with no
 * further residual evaluation: there is no refined mode to turn on, and Q_REFINE stays refused.  The calls, their
 * host and device forms, MAX_SIZE_QSPACE, SVD_THRESH and the statistics are the f64 instance's;
 * IterativeSolverHbmQStorage reports 4.  Refused by name: an algorithm other than "DIIS", an instance with more
 * than one rank, a P space (IterativeSolverAddP), and Q_STORAGE=f32 over a vector library without the
 * mixed-precision ABI.
 *
 * Linear equations.  IterativeSolverLinearEquationsInitialize accepts Q_STORAGE=f32 and, with it, Q_REFINE=1 and
 * Q_REFINE_KAPPA (one rank, "Davidson").  Plain: the right-hand sides are stored rounded with the Q space, so the
 * true residual cannot fall below about 2^-24 |b|: thresholds down to about 1e-6.  Refined: the instance keeps an
 * f64 twin of every right-hand side, which the subspace and the residuals read instead; the refine action, the
 * rounded rows of EndIteration and the statistics are the ones described here, and the reported errors are true
 * relative residuals down to f64 thresholds.  Refused by name: Q_REFINE=1 without Q_STORAGE=f32 (with the Q space
 * in f64 the residuals are exact already), Q_REFINE_DSPACE, and in refined mode hermitian = 0, MAX_SIZE_QSPACE,
 * RESET_D, RESET_D_MAX_Q_SIZE and aughes > 0 (the augmented Hessian's residual is not A x - b).
 *
 * The refine action.  fn(nvec, parameters, action, ld, user) must set action row k = H * parameters row k for
 * k < nvec (row k at p + k*ld).  It is called from inside IterativeSolverAddVector, its device form and
 * IterativeSolverAddP, at most once per batch of roots, with nvec <= the call's buffer_size, and its two arrays
 * ARE that call's own `parameters` and `action`: the layer writes the nvec selected solutions, compacted, into
 * rows [0, nvec) of `parameters`, calls fn, and reads rows [0, nvec) of `action`.  For a host call ld =
 * dimension and the arrays are host memory; for a device call ld is the call's ld, both are device memory and
 * the stream contract is that of the device forms (fn's work ordered on the context stream, or finished, when
 * it returns).  The call then completes and writes every row of both arrays as it always does, so the caller's
 * arrays end as they would without a refinement; no other memory is used.  A refinement that is needed while no
 * action is set is an error naming this call.
 *
 * Rounding before the action.  The scheme rests on a_j = H q_j holding for the vector q_j the Q space STORES,
 * so with Q_STORAGE=f32 and Q_REFINE the first `result` parameter rows IterativeSolverEndIteration (and its
 * device form) returns are rounded to binary32-representable values, (double)(float)(s*x) -- on the device
 * route by the export itself (ssp_rows_export_quantised), at no extra pass.  The remaining rows and every
 * residual row are as without the option.  The initial guess is the caller's: unit vectors need nothing; any
 * other guess goes through IterativeSolverHbmQuantise[Device] before its action is formed.  A guess that is not
 * representable leaves the stored pair (q, a) inconsistent at 2^-24 |H|: the solve then stalls above the
 * threshold; it does not report a false residual, because refined errors are true ones.
 *
 * Diagonals.  With actions stored rounded, the residual of a unit-vector guess is rounding noise at the guess's
 * index (2^-24 |a|, where f64 arithmetic gives an exact zero), and the usual preconditioner r / ((d - theta) +
 * 1e-15) must not meet it with an exact zero denominator.  The C++ solve() keeps the problem's diagonals in a Q
 * vector; an instance with Q_STORAGE=f32 does the same: IterativeSolverSetDiagonals[Device] rounds them to the Q
 * storage, and IterativeSolverDiagonals[Device] returns them so.  A caller that holds its own diagonals
 * preconditions with their rounded values, or regularises its denominator. */
typedef void (*itsolv_refine_action_fn)(size_t nvec, const double* parameters, double* action, size_t ld, void* user);
/* The refine action of the top instance; NULL clears it.  Returns 0, or 1 (IterativeSolverHbmLastError). */
int IterativeSolverHbmSetRefineAction(itsolv_refine_action_fn fn, void* user);
/* Of the top instance: actions spent on refined residuals, the iteration (from 1) of the first (0: none), the
 * largest delta (the bound on |estimate - true residual|) of the last iteration.  Returns 0; 1: no instance. */
int IterativeSolverHbmRefineStatistics(int* refined_actions, int* first_refined_iteration, double* max_delta);
/* Of the top instance with Q_REFINE_DSPACE=1: the rebuilds of its D space and the actions spent on them (these
 * are not among the refined_actions above).  Returns 0; 1: no instance. */
int IterativeSolverHbmRefineDspaceStats(int* rebuilds, int* actions);
/* Bytes per stored Q element of the top instance: 8 or 4; 0 when there is none. */
size_t IterativeSolverHbmQStorage(void);
/* Rounds `buffer_size` parameter rows in place to the Q storage format of the top instance (host rows of
 * length `dimension`; device rows of this rank's shard, row k at p + k*ld).  Returns the number of rows
 * rounded: 0 with Q_STORAGE=f64, where there is nothing to round. */
size_t IterativeSolverHbmQuantise(size_t buffer_size, double* parameters);
size_t IterativeSolverHbmQuantiseDevice(size_t buffer_size, double* parameters, size_t ld);

#ifdef __cplusplus
}
#endif
#endif
