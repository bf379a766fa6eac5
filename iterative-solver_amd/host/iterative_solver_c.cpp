// The reference's reverse-communication C API (src/molpro/linalg/IterativeSolverC.h:6-73,
// IterativeSolverCMPI.cpp:158-534) over the HBM handlers: R arrives as host arrays and is staged
// into HBM vectors for each call; Q, D and every subspace operation stay on the device.
#include "iterative_solver_c.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "itsolv_hbm/hbm_handlers.h"
#include "itsolv_hbm/solver_factory.h"
#include "itsolv_hbm/solvers.h"
#include "mpi_bridge.h"
#include "rc_solver.h"

using molpro::linalg::hbm::check;
using molpro::linalg::hbm::Device;
using molpro::linalg::hbm::SparseP;
using molpro::linalg::hbm::Vec;
namespace it = molpro::linalg::itsolv;

// Weak references (null when the loaded vector library lacks them): see import_rows below.
extern "C" {
int ssp_rows_import(ssp_ctx*, const double*, size_t, double* const*, int, size_t) __attribute__((weak));
int ssp_rows_export(ssp_ctx*, const double* const*, const double*, int, double*, size_t, size_t) __attribute__((weak));
int ssp_rows_export_quantised(ssp_ctx*, const double* const*, const double*, int, int, double*, size_t, size_t)
    __attribute__((weak));
}

namespace {

const auto rows_import_fn = &ssp_rows_import;
const auto rows_export_fn = &ssp_rows_export;
const auto rows_export_q_fn = &ssp_rows_export_quantised;
const auto make_q32_fn = &itsolv_rc::make_rc_davidson_q32;  // null without host_q32/ (rc_solver.h)
const auto make_lineq_q32_fn = &itsolv_rc::make_rc_linear_equations_q32;  // the same
const auto make_diis_q32_fn = &itsolv_rc::make_rc_diis_q32;                // the same

using Solver = it::IterativeSolverTemplate<Vec, Vec, SparseP>;
using Davidson = it::LinearEigensystemDavidson<Vec, Vec, SparseP>;
using RSPT = it::LinearEigensystemRSPT<Vec, Vec, SparseP>;
using DIIS = it::NonLinearEquationsDIIS<Vec, Vec, SparseP>;
using LinEq = it::LinearEquationsDavidson<Vec, Vec, SparseP>;
using BFGS = it::OptimizeBFGS<Vec, Vec, SparseP>;
using SD = it::OptimizeSD<Vec, Vec, SparseP>;
typedef void (*Apply_on_p_fort)(const double*, double*, const size_t, const size_t*);

thread_local std::string g_error;
ssp_ctx* g_user_ctx = nullptr;
bool g_throw = true;

struct Instance {
  uint64_t id = 0;  // IterativeSolverHbmInstanceId: lets a binding finalize its own instance
  std::shared_ptr<Device> dev;
  std::unique_ptr<itsolv_rc::RcSolver> solver;  // the Q-independent face: Q is Vec, or VecF32 (Q_STORAGE=f32)
  size_t dimension = 0, offset = 0, local = 0;
  std::vector<Vec> rp, ra;  // HBM staging of the caller's R vectors (grown on demand)
  Apply_on_p_fort apply_on_p_fort = nullptr;
  std::unique_ptr<Vec> diagonals;
  bool has_values = false;
  bool has_eigenvalues = false;
  // refined mode (Q_REFINE): the caller's action, and the arrays of the running AddVector / AddP call that
  // serve as its scratch (RefineScratch below)
  itsolv_refine_action_fn refine_fn = nullptr;
  void* refine_user = nullptr;
  double *scratch_p = nullptr, *scratch_a = nullptr;
  size_t scratch_ld = 0;
  size_t scratch_rows = 0;
  bool scratch_device = false;
};
// The instance stack (reference IterativeSolverCMPI.cpp: std::stack<Instance>); the back is the top,
// the only active instance.  A vector, so that IterativeSolverHbmFinalizeInstance can also remove
// an instance below the top whose owner has gone away.  Instances are heap-held: the P-space
// callback keeps a pointer to its instance across pushes and erasures.
std::vector<std::unique_ptr<Instance>> instances;
uint64_t g_next_id = 1;

Instance& top() {
  if (instances.empty()) throw std::runtime_error("IterativeSolver not initialised properly");
  return *instances.back();
}
void push(Instance&& in) {
  in.id = g_next_id++;
  instances.push_back(std::make_unique<Instance>(std::move(in)));
}

// Without IterativeSolverHbmSetContext the node-local rank a launcher exports (torchrun, Open MPI,
// MPICH, Slurm) picks the device, so independent processes on one node spread over its GPUs
// instead of all landing on device 0.
int default_device() {
  for (const char* var : {"LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "MPI_LOCALRANKID", "SLURM_LOCALID"}) {
    const char* s = std::getenv(var);
    if (!s || !*s) continue;
    const int r = std::atoi(s), n = ssp_device_count();
    return (r >= 0 && n > 0) ? r % n : 0;
  }
  return 0;
}

// A context attached to the ranks of an MPI communicator (mpi_bridge.h), with the transport's state.
class BridgedDevice : public Device {
 public:
  BridgedDevice(int device, int64_t fcomm) : Device(device) {
    m_link = molpro::linalg::hbm::mpi::attach(ctx(), fcomm, nullptr);
  }

 private:
  std::shared_ptr<void> m_link;
};
// One bridged context per communicator, shared by the instances that use it and released with the
// last of them (every rank creates and finalizes instances in the same order, so the collective
// attach happens on all ranks together).
std::map<int64_t, std::weak_ptr<Device>> g_bridged;

// The instance's device and ranks.  In order:
//  - the context set by IterativeSolverHbmSetContext;
//  - the communicator fcomm names, when the process has an initialised MPI library (reference
//    IterativeSolverCMPI.cpp:169, :205, :234, :254 -- MPI_Comm_f2c(fcomm)): a context attached to its
//    ranks, on the device of the rank's place among them on its node (one rank: a private context);
//  - otherwise a private single-rank context on the node-local rank's device.
std::shared_ptr<Device> make_device(int64_t fcomm) {
  namespace mpi = molpro::linalg::hbm::mpi;
  if (g_user_ctx) return std::make_shared<Device>(g_user_ctx, true);
  mpi::Bridge* b = mpi::bridge();
  if (b && b->active() && b->valid(fcomm)) {
    if (b->size(fcomm) <= 1) return std::make_shared<Device>(mpi::device_for(fcomm));
    if (auto d = g_bridged[fcomm].lock()) return d;
    auto d = std::make_shared<BridgedDevice>(mpi::device_for(fcomm), fcomm);
    g_bridged[fcomm] = d;
    return d;
  }
  return std::make_shared<Device>(default_device());
}

void setup(Instance& in, size_t n, size_t* range_begin, size_t* range_end) {
  in.dimension = n;
  std::tie(in.offset, in.local) = in.dev->shard(n);
  // reference DistrArrayDefaultRange (IterativeSolverCMPI.cpp:80-89)
  if (range_begin) *range_begin = in.offset;
  if (range_end) *range_end = in.offset + in.local;
}

void ensure_r(Instance& in, size_t nvec) {
  while (in.rp.size() < nvec) {
    in.rp.emplace_back(in.dev, in.dimension);
    in.ra.emplace_back(in.dev, in.dimension);
  }
}

// This rank's range of host vectors [k*dimension + offset, +local) <-> HBM.
void upload(Instance& in, std::vector<Vec>& v, size_t nvec, const double* host) {
  for (size_t k = 0; k < nvec; ++k)
    check(ssp_upload(in.dev->ctx(), v[k].data_wo(), host + k * in.dimension + in.offset, in.local), "ssp_upload");
}
void download(Instance& in, std::vector<Vec>& v, size_t nvec, double* host) {
  for (size_t k = 0; k < nvec; ++k)
    check(ssp_download(in.dev->ctx(), host + k * in.dimension + in.offset, v[k].data(), in.local), "ssp_download");
}

// Device rows [dev + k*ld, +local) <-> HBM staging, one pass each way (the device forms below).  The
// row-block entry points are referenced weakly: this file is also linked against the CPU emulation of
// the f64 C ABI, which has none, and then (or over an older library) the rows move one by one --
// ssp_copy for a 16-byte aligned row, ssp_scal_copy where a scale is pending -- and a misaligned row is
// refused, before anything is staged.
void check_rows(const Instance& in, size_t nvec, const double* dev, size_t ld, bool have_kernel, const char* what) {
  if (nvec == 0 || in.local == 0) return;
  if (!dev) throw std::invalid_argument(std::string(what) + ": null device pointer");
  if (ld < in.local) throw std::invalid_argument(std::string(what) + ": ld smaller than this rank's range");
  if (have_kernel) return;
  for (size_t k = 0; k < nvec; ++k)
    if (reinterpret_cast<uintptr_t>(dev + k * ld) % 16 != 0)
      throw std::logic_error(std::string(what) + ": SSP_ERR_UNSUPPORTED: row " + std::to_string(k) +
                             " is not 16-byte aligned and the loaded library has no ssp_rows_import / "
                             "ssp_rows_export");
}
void import_rows(Instance& in, std::vector<Vec>& v, size_t nvec, const double* dev, size_t ld) {
  if (nvec == 0 || in.local == 0) return;
  std::vector<double*> dst(nvec);
  for (size_t k = 0; k < nvec; ++k) dst[k] = v[k].data_wo();
  if (rows_import_fn) {
    check(rows_import_fn(in.dev->ctx(), dev, ld, dst.data(), int(nvec), in.local), "ssp_rows_import");
    return;
  }
  for (size_t k = 0; k < nvec; ++k) check(ssp_copy(in.dev->ctx(), dst[k], dev + k * ld, in.local), "ssp_copy");
}
// mq > 0: the first mq rows are rounded to the Q storage format as they are stored (the caller has checked
// that the loaded library has the export that rounds).
void export_list(Instance& in, const std::vector<const Vec*>& v, double* dev, size_t ld, size_t mq = 0) {
  const size_t nvec = v.size();
  if (nvec == 0 || in.local == 0) return;
  std::vector<const double*> src(nvec);
  std::vector<double> xs(nvec);
  for (size_t k = 0; k < nvec; ++k) {
    src[k] = v[k]->data_deferred();
    xs[k] = v[k]->scale();
  }
  if (mq > 0) {
    check(rows_export_q_fn(in.dev->ctx(), src.data(), xs.data(), int(nvec), int(mq), dev, ld, in.local),
          "ssp_rows_export_quantised");
    return;
  }
  if (rows_export_fn) {
    check(rows_export_fn(in.dev->ctx(), src.data(), xs.data(), int(nvec), dev, ld, in.local), "ssp_rows_export");
    return;
  }
  for (size_t k = 0; k < nvec; ++k) {
    if (xs[k] == 1.0) check(ssp_copy(in.dev->ctx(), dev + k * ld, src[k], in.local), "ssp_copy");
    else check(ssp_scal_copy(in.dev->ctx(), xs[k], dev + k * ld, src[k], in.local), "ssp_scal_copy");
  }
}
void export_rows(Instance& in, const std::vector<Vec>& v, size_t nvec, double* dev, size_t ld, size_t mq = 0) {
  std::vector<const Vec*> list(nvec);
  for (size_t k = 0; k < nvec; ++k) list[k] = &v[k];
  export_list(in, list, dev, ld, mq);
}
// Both arrays of a device call, checked before either is staged.
void check_pair(const Instance& in, size_t nvec, const double* a, const double* b, size_t ld, const char* what) {
  const bool have = rows_import_fn && rows_export_fn;
  check_rows(in, nvec, a, ld, have, what);
  check_rows(in, nvec, b, ld, have, what);
}

// reference DistrArraySynchronize / gather_all (IterativeSolverCMPI.cpp:133-139): every rank
// receives every rank's range of each vector.
void synchronize(Instance& in, size_t nvec, double* host) {
  const int nr = in.dev->nranks();
  if (nr <= 1 || nvec == 0) return;
  const size_t chunk = (in.dimension + size_t(nr) - 1) / size_t(nr);  // >= the largest shard
  std::vector<double> send(chunk), recv(chunk * size_t(nr));
  for (size_t k = 0; k < nvec; ++k) {
    double* vec = host + k * in.dimension;
    std::memcpy(send.data(), vec + in.offset, in.local * sizeof(double));
    check(ssp_allgather_host(in.dev->ctx(), send.data(), recv.data(), chunk * sizeof(double)), "ssp_allgather_host");
    for (int r = 0; r < nr; ++r) {
      size_t off = 0, len = 0;
      check(ssp_shard_range(in.dimension, nr, r, &off, &len), "ssp_shard_range");
      std::memcpy(vec + off, recv.data() + size_t(r) * chunk, len * sizeof(double));
    }
  }
}

it::VecRef<Vec> first(std::vector<Vec>& v, size_t n) { return it::wrap(v.begin(), v.begin() + long(n)); }

// ---- refined mode (Q_REFINE; include/iterative_solver_c.h) ------------------------------------------------
// The arrays of the running AddVector / AddVectorDevice / AddP call are the scratch of a refinement inside it:
// the call exports every row at its end, so what the refinement leaves in them is overwritten.  So are the two
// arrays of an EndIteration / EndIterationDevice call once they are imported: the scratch of a D-space rebuild
// (Q_REFINE_DSPACE) inside it.  rows: how many rows the arrays hold.
struct RefineScratch {
  Instance& in;
  RefineScratch(Instance& i, double* p, double* a, size_t ld, bool device, size_t rows) : in(i) {
    in.scratch_p = p;
    in.scratch_a = a;
    in.scratch_ld = ld;
    in.scratch_rows = rows;
    in.scratch_device = device;
  }
  ~RefineScratch() { in.scratch_p = in.scratch_a = nullptr; }
};

// The solver's refine action (DavidsonSolver::set_refine_action): the m selected solutions, compacted,
// into rows [0, m) of the call's parameters (pending scales applied), the caller's action on them, rows [0, m)
// of its action array into the solver's vectors.
void refine_action(Instance& in, const it::CVecRef<Vec>& x, const it::VecRef<Vec>& a) {
  const size_t m = x.size();
  if (!in.refine_fn || !in.scratch_p || !in.scratch_a)
    throw std::logic_error("refine: no IterativeSolverHbmSetRefineAction callback for this call");
  if (m > in.scratch_rows)
    throw std::logic_error("refine: the call's arrays hold " + std::to_string(in.scratch_rows) + " rows, the action needs " +
                           std::to_string(m));
  double* const p = in.scratch_p;
  double* const g = in.scratch_a;
  const size_t ld = in.scratch_ld;
  if (in.scratch_device) {
    std::vector<const Vec*> src(m);
    for (size_t k = 0; k < m; ++k) src[k] = &x[k].get();
    export_list(in, src, p, ld);
    in.refine_fn(m, p, g, ld, in.refine_user);
    if (in.local == 0) return;
    std::vector<double*> dst(m);
    for (size_t k = 0; k < m; ++k) dst[k] = a[k].get().data_wo();
    if (rows_import_fn) {
      check(rows_import_fn(in.dev->ctx(), g, ld, dst.data(), int(m), in.local), "ssp_rows_import");
    } else {
      for (size_t k = 0; k < m; ++k) check(ssp_copy(in.dev->ctx(), dst[k], g + k * ld, in.local), "ssp_copy");
    }
    return;
  }
  for (size_t k = 0; k < m; ++k)
    check(ssp_download(in.dev->ctx(), p + k * ld + in.offset, x[k].get().data(), in.local), "ssp_download");
  in.refine_fn(m, p, g, ld, in.refine_user);
  for (size_t k = 0; k < m; ++k)
    check(ssp_upload(in.dev->ctx(), a[k].get().data_wo(), g + k * ld + in.offset, in.local), "ssp_upload");
}

// Whether EndIteration returns its new parameter rows rounded to the Q storage format: the refined mode over
// a Q space narrower than R (what solve() does before problem.action, refine.h step 1).
bool rounds_new_parameters(const Instance& in) {
  return in.solver->refine_options().on && in.solver->q_bytes() < sizeof(double);
}

// solve() keeps the problem's diagonals in a Q vector; so does an instance whose Q space is narrower than R.
// It matters: with actions stored rounded, the residual of a unit-vector guess is rounding noise (not an exact
// zero) at the guess's index, and the default preconditioner divides it by (d - theta) + 1e-15 -- which must
// then not be the exact zero the f64 diagonal would give.
void store_diagonals_as_q(Instance& in) {
  if (in.solver->q_bytes() < sizeof(double) && in.diagonals) in.solver->quantise(it::wrap_arg(*in.diagonals));
}

// Q_STORAGE, Q_REFINE, Q_REFINE_KAPPA, Q_REFINE_DSPACE, Q_REFINE_DSPACE_SLACK of an options string (keys
// upper-cased by parse_options).
struct QOptions {
  bool f32 = false, refine = false, named = false, dspace = false;
  double kappa = 8.0;
  int dspace_slack = -1;  // the solver's rule
};
QOptions q_options(const char* options) {
  QOptions q;
  const auto m = it::parse_options(options ? options : "");
  const it::util::StringFacet facet;
  if (auto f = m.find("Q_STORAGE"); f != m.end()) {
    const auto v = facet.tolower(f->second);
    if (v != "f32" && v != "f64") throw std::invalid_argument("Q_STORAGE=" + f->second + ": must be f64 or f32");
    q.f32 = v == "f32";
    q.named = q.named || q.f32;
  }
  if (auto f = m.find("Q_REFINE"); f != m.end()) {
    q.refine = facet.tobool(f->second);
    q.named = q.named || q.refine;
  }
  if (auto f = m.find("Q_REFINE_KAPPA"); f != m.end()) {
    if (!q.refine) throw std::invalid_argument("Q_REFINE_KAPPA: needs Q_REFINE=1");
    q.kappa = std::stod(f->second);
    if (!(q.kappa > 0)) throw std::invalid_argument("Q_REFINE_KAPPA=" + f->second + ": must be positive");
  }
  if (auto f = m.find("Q_REFINE_DSPACE"); f != m.end()) {
    q.dspace = facet.tobool(f->second);
    if (q.dspace && !q.refine) throw std::invalid_argument("Q_REFINE_DSPACE: needs Q_REFINE=1");
  }
  if (auto f = m.find("Q_REFINE_DSPACE_SLACK"); f != m.end()) {
    if (!q.dspace) throw std::invalid_argument("Q_REFINE_DSPACE_SLACK: needs Q_REFINE_DSPACE=1");
    q.dspace_slack = std::stoi(f->second);
    if (q.dspace_slack < 0) throw std::invalid_argument("Q_REFINE_DSPACE_SLACK=" + f->second + ": must not be negative");
  }
  return q;
}
// The families that have neither option.
void refuse_q_options(const char* options, const char* family) {
  const auto q = q_options(options);
  if (q.f32) throw std::invalid_argument(std::string("Q_STORAGE=f32: not available for ") + family);
  if (q.refine) throw std::invalid_argument(std::string("Q_REFINE: not available for ") + family);
}

std::unique_ptr<itsolv_rc::RcSolver> face(std::unique_ptr<Solver> solver,
                                          std::shared_ptr<it::ArrayHandlers<Vec, Vec, SparseP>> handlers) {
  return std::make_unique<itsolv_rc::RcSolverOf<Vec>>(std::move(solver), std::move(handlers));
}

// add_vector on the staged R vectors (IterativeSolverAddVector and its device form).
// Non-linear solvers take one vector through their own add_vector (for DIIS: the residual norm,
// the convergence flag and the least-important-vector deletion, NonLinearEquationsDIIS.h:83-102),
// as IterativeSolverTemplate::solve does for them (:379-382).  The reference's C layer reaches
// the generic vector-list overload instead, which skips that logic.
size_t add_vector_staged(Instance& in, size_t buffer_size) {
  return in.solver->nonlinear() && buffer_size >= 1
             ? size_t(in.solver->add_vector(in.rp[0], in.ra[0], 0.0))
             : size_t(in.solver->add_vector(first(in.rp, buffer_size), first(in.ra, buffer_size)));
}

it::Verbosity verbosity_of(int v) {
  return v <= 0 ? it::Verbosity::None : v == 1 ? it::Verbosity::Summary : v == 2 ? it::Verbosity::Iteration
                                                                                : it::Verbosity::Detailed;
}

// Runs one API call.  Errors are thrown as the reference's extern "C" functions throw; with
// IterativeSolverHbmSetThrow(0) they are recorded for IterativeSolverHbmLastError() instead and the
// call returns a zero value (for callers that cannot unwind C++ exceptions: ctypes, Fortran).
template <class F>
auto guarded(F&& f) -> decltype(f()) {
  using T = decltype(f());
  g_error.clear();
  try {
    return f();
  } catch (const std::exception& e) {
    g_error = e.what();
    if (g_throw) throw;
  }
  if constexpr (!std::is_void_v<T>) return T{};
}

molpro::linalg::hbm::mpi::Bridge* active_mpi() {
  auto* b = molpro::linalg::hbm::mpi::bridge();
  return b && b->active() ? b : nullptr;
}

}  // namespace

extern "C" {

int IterativeSolverHbmSetThrow(int enable) {
  g_throw = enable != 0;
  return 0;
}

int IterativeSolverHbmSetContext(ssp_ctx* ctx) {
  g_error.clear();  // (a call that cannot fail: it does not leave the error of a refused Initialize before it standing)
  g_user_ctx = ctx;
  return 0;
}

const char* IterativeSolverHbmLastError(void) { return g_error.c_str(); }

int IterativeSolverHbmStatistics(int* iterations, int* r_creations, int* q_creations) {
  if (instances.empty()) return 1;
  const auto& s = instances.back()->solver->statistics();
  if (iterations) *iterations = s.iterations;
  if (r_creations) *r_creations = s.r_creations;
  if (q_creations) *q_creations = s.q_creations;
  return 0;
}

void IterativeSolverLinearEigensystemInitialize(size_t nQ, size_t nroot, size_t* range_begin, size_t* range_end,
                                                double thresh, double thresh_value, int hermitian, int verbosity,
                                                const char* fname, int64_t fcomm, const char* algorithm,
                                                const char* options) {
  guarded([&] {
    (void)fname;
    Instance in;
    in.dev = make_device(fcomm);
    const std::string method = algorithm ? algorithm : "";
    const auto q = q_options(options);
    if (q.named) {  // extension: the Q space in f32 and / or refined residuals, one-rank Davidson only
      const char* which = q.f32 ? "Q_STORAGE=f32" : q.dspace ? "Q_REFINE_DSPACE" : "Q_REFINE";
      if (!(method == "Davidson" || method.empty()))
        throw std::invalid_argument(std::string(which) + ": available for the LinearEigensystem Davidson only, not " + method);
      if (in.dev->nranks() > 1)
        throw std::invalid_argument(std::string(which) + ": not available on an instance with more than one rank");
      if (q.f32 && !make_q32_fn)
        throw std::logic_error("Q_STORAGE=f32: SSP_ERR_UNSUPPORTED: the loaded vector library has no mixed-precision ABI");
    }
    // method dispatch and option parsing as the reference's create_LinearEigensystem (SolverFactory.h:114-125)
    if (q.f32) {  // the same construction over make_handlers_q32() (host_q32/rc_q32.cpp)
      in.solver = make_q32_fn(options ? options : "", nroot, hermitian != 0);
    } else {
      auto handlers = molpro::linalg::hbm::make_handlers();
      auto solver = it::create_LinearEigensystem(method, options ? options : "", handlers);
      solver->set_n_roots(nroot);  // every method (reference IterativeSolverCMPI.cpp:176)
      if (auto* d = dynamic_cast<Davidson*>(solver.get())) d->set_hermiticity(hermitian != 0);
      in.solver = face(std::move(solver), std::move(handlers));
    }
    in.solver->set_verbosity(verbosity_of(verbosity));
    in.solver->set_convergence_threshold(thresh);
    in.solver->set_convergence_threshold_value(thresh_value);
    // the refined mode's scope is checked here, not in the middle of a solve: hermitian = 0, MAX_SIZE_QSPACE,
    // RESET_D and RESET_D_MAX_Q_SIZE are errors naming the option (Q_REFINE_DSPACE=1 admits MAX_SIZE_QSPACE)
    if (q.refine) in.solver->set_refine(it::RefineOptions{true, q.kappa, q.dspace, q.dspace_slack});
    in.has_eigenvalues = true;
    setup(in, nQ, range_begin, range_end);
    push(std::move(in));
  });
}

void IterativeSolverLinearEquationsInitialize(size_t n, size_t nroot, size_t* range_begin, size_t* range_end,
                                              const double* rhs, double aughes, double thresh, double thresh_value,
                                              int hermitian, int verbosity, const char* fname, int64_t fcomm,
                                              const char* algorithm, const char* options) {
  guarded([&] {
    (void)fname;
    // extension: Q_STORAGE=f32, and with it Q_REFINE=1 and Q_REFINE_KAPPA (one rank, "Davidson").  Q_REFINE=1
    // alone stays refused: with the Q space in f64 the residuals are exact already.
    const auto q = q_options(options);
    const std::string method = algorithm ? algorithm : "";
    if (q.dspace) throw std::invalid_argument("Q_REFINE_DSPACE: not available for LinearEquations");
    if (q.refine && !q.f32)
      throw std::invalid_argument("Q_REFINE: not available for LinearEquations unless Q_STORAGE=f32 (with the Q space "
                                  "in f64 the residuals are exact already)");
    if (q.f32 && !(method == "Davidson" || method.empty()))
      throw std::invalid_argument("Q_STORAGE=f32: available for the LinearEquations Davidson only, not " + method);
    if (q.f32 && !make_lineq_q32_fn)
      throw std::logic_error("Q_STORAGE=f32: SSP_ERR_UNSUPPORTED: not available for LinearEquations here: the loaded "
                             "vector library has no mixed-precision ABI");
    Instance in;
    in.dev = make_device(fcomm);
    if (q.f32 && in.dev->nranks() > 1)
      throw std::invalid_argument("Q_STORAGE=f32: LinearEquations: not available on an instance with more than one rank");
    setup(in, n, range_begin, range_end);
    // reference IterativeSolverCMPI.cpp:199-225: rhs as R vectors, then options
    std::vector<Vec> b;
    for (size_t r = 0; r < nroot; ++r) {
      b.emplace_back(in.dev, n);
      check(ssp_upload(in.dev->ctx(), b.back().data_wo(), rhs + r * n + in.offset, in.local), "ssp_upload");
    }
    if (q.f32) {  // the same construction over make_handlers_q32() (host_q32/rc_q32.cpp)
      in.solver = make_lineq_q32_fn(options ? options : "", b, hermitian != 0, aughes, it::RefineOptions{q.refine, q.kappa});
      in.solver->set_convergence_threshold(thresh);
      in.solver->set_convergence_threshold_value(thresh_value);
      in.solver->set_verbosity(verbosity_of(verbosity));
      push(std::move(in));
      return;
    }
    auto handlers = molpro::linalg::hbm::make_handlers();
    auto made = it::create_LinearEquations(algorithm ? algorithm : "", options ? options : "", handlers);
    std::unique_ptr<LinEq> solver(static_cast<LinEq*>(made.release()));
    solver->set_hermiticity(hermitian != 0);
    solver->set_n_roots(nroot);
    solver->add_equations(b);
    solver->set_convergence_threshold(thresh);
    solver->set_convergence_threshold_value(thresh_value);
    if (aughes > 0) solver->set_augmented_hessian(aughes);
    solver->set_verbosity(verbosity_of(verbosity));
    in.solver = face(std::move(solver), std::move(handlers));
    push(std::move(in));
  });
}

void IterativeSolverNonLinearEquationsInitialize(size_t n, size_t* range_begin, size_t* range_end, double thresh,
                                                 int verbosity, const char* fname, int64_t fcomm,
                                                 const char* algorithm, const char* options) {
  guarded([&] {
    (void)fname;
    // extension: Q_STORAGE=f32 (one rank, "DIIS"): the history as f32 differences behind f64 anchors, which needs
    // no refinement -- Q_REFINE stays refused
    const auto q = q_options(options);
    const std::string method = algorithm ? algorithm : "";
    if (q.refine) throw std::invalid_argument("Q_REFINE: not available for NonLinearEquations");
    if (q.f32 && !(method == "DIIS" || method.empty()))
      throw std::invalid_argument("Q_STORAGE=f32: available for the NonLinearEquations DIIS only, not " + method);
    if (q.f32 && !make_diis_q32_fn)
      throw std::logic_error("Q_STORAGE=f32: SSP_ERR_UNSUPPORTED: not available for NonLinearEquations here: the loaded "
                             "vector library has no mixed-precision ABI");
    Instance in;
    in.dev = make_device(fcomm);
    if (q.f32 && in.dev->nranks() > 1)
      throw std::invalid_argument("Q_STORAGE=f32: NonLinearEquations: not available on an instance with more than one rank");
    if (q.f32) {  // the same construction over make_handlers_q32() (host_q32/rc_q32.cpp)
      in.solver = make_diis_q32_fn(options ? options : "");
      in.solver->set_convergence_threshold(thresh);
      in.solver->set_verbosity(verbosity_of(verbosity));
      setup(in, n, range_begin, range_end);
      push(std::move(in));
      return;
    }
    auto handlers = molpro::linalg::hbm::make_handlers();
    auto solver = it::create_NonLinearEquations(algorithm ? algorithm : "", options ? options : "", handlers);
    solver->set_convergence_threshold(thresh);
    solver->set_verbosity(verbosity_of(verbosity));
    in.solver = face(std::move(solver), std::move(handlers));
    setup(in, n, range_begin, range_end);
    push(std::move(in));
  });
}

void IterativeSolverOptimizeInitialize(size_t n, size_t* range_begin, size_t* range_end, double thresh,
                                       double thresh_value, int verbosity, int minimize, const char* fname,
                                       int64_t fcomm, const char* algorithm, const char* options) {
  guarded([&] {
    (void)fname;
    (void)minimize;  // ignored, as the reference does (IterativeSolverCMPI.cpp:250-268)
    refuse_q_options(options, "Optimize");
    Instance in;
    in.dev = make_device(fcomm);
    auto handlers = molpro::linalg::hbm::make_handlers();
    auto solver = it::create_Optimize(algorithm ? algorithm : "", options ? options : "", handlers);
    // reference IterativeSolverCMPI.cpp:245-264
    solver->set_n_roots(1);
    solver->set_convergence_threshold(thresh);
    solver->set_convergence_threshold_value(thresh_value);
    solver->set_verbosity(verbosity_of(verbosity));
    in.solver = face(std::move(solver), std::move(handlers));
    in.has_values = true;
    setup(in, n, range_begin, range_end);
    push(std::move(in));
  });
}

void IterativeSolverFinalize(void) {
  guarded([] {
    if (!instances.empty()) instances.pop_back();
  });
}

uint64_t IterativeSolverHbmInstanceId(void) { return instances.empty() ? 0 : instances.back()->id; }

int IterativeSolverHbmFinalizeInstance(uint64_t id) {
  for (auto it = instances.begin(); it != instances.end(); ++it)
    if ((*it)->id == id) {
      instances.erase(it);
      return 0;
    }
  return 1;
}

size_t IterativeSolverAddVector(size_t buffer_size, double* parameters, double* action, int sync) {
  return guarded([&] {
    auto& in = top();
    ensure_r(in, buffer_size);
    upload(in, in.rp, buffer_size, parameters);
    upload(in, in.ra, buffer_size, action);
    const RefineScratch scratch(in, parameters, action, in.dimension, false, buffer_size);
    const size_t nwork = add_vector_staged(in, buffer_size);
    // The reference's R vectors are views of these host arrays, so every vector the solver wrote
    // (solutions and residuals of all roots, batch by batch) reaches the caller; sync gathers the
    // working set (IterativeSolverCMPI.cpp:302-306).
    download(in, in.rp, buffer_size, parameters);
    download(in, in.ra, buffer_size, action);
    const size_t nws = std::min(in.solver->working_set().size(), buffer_size);
    if (sync) {
      synchronize(in, nws, parameters);
      synchronize(in, nws, action);
    }
    return nwork;
  });
}

void IterativeSolverSolution(int nroot, int* roots, double* parameters, double* action, int sync) {
  guarded([&] {
    auto& in = top();
    const size_t n = size_t(nroot);
    ensure_r(in, n);
    std::vector<int> r(roots, roots + nroot);
    in.solver->solution(r, first(in.rp, n), first(in.ra, n));
    download(in, in.rp, n, parameters);
    download(in, in.ra, n, action);
    if (sync) {
      synchronize(in, n, parameters);
      synchronize(in, n, action);
    }
  });
}

size_t IterativeSolverAddValue(double value, double* parameters, double* action, int sync) {
  return guarded([&]() -> size_t {
    auto& in = top();
    ensure_r(in, 1);
    upload(in, in.rp, 1, parameters);
    upload(in, in.ra, 1, action);
    // reference IterativeSolverCMPI.cpp:270-298: working set of one, or none when line-searching
    const int r = in.solver->add_vector(in.rp[0], in.ra[0], value);
    download(in, in.rp, 1, parameters);
    download(in, in.ra, 1, action);
    if (sync) {
      synchronize(in, 1, parameters);
      synchronize(in, 1, action);
    }
    return r > 0 ? 1 : 0;
  });
}

size_t IterativeSolverEndIteration(size_t buffer_size, double* solution, double* residual, int sync) {
  return guarded([&] {
    auto& in = top();
    ensure_r(in, buffer_size);
    upload(in, in.rp, buffer_size, solution);
    upload(in, in.ra, buffer_size, residual);
    const RefineScratch scratch(in, solution, residual, in.dimension, false, buffer_size);  // a D-space rebuild's
    const size_t result = in.solver->end_iteration(first(in.rp, buffer_size), first(in.ra, buffer_size));
    if (rounds_new_parameters(in)) in.solver->quantise(first(in.rp, std::min(result, buffer_size)));
    download(in, in.rp, buffer_size, solution);
    download(in, in.ra, buffer_size, residual);
    const size_t nws = std::min(in.solver->working_set().size(), buffer_size);
    if (sync) {
      synchronize(in, nws, solution);
      synchronize(in, nws, residual);
    }
    return result;
  });
}

int IterativeSolverEndIterationNeeded(void) {
  return guarded([] { return top().solver->end_iteration_needed() ? 1 : 0; });
}

size_t IterativeSolverAddP(size_t buffer_size, size_t nP, const size_t* offsets, const size_t* indices,
                           const double* coefficients, const double* pp, double* parameters, double* action, int sync,
                           void (*func)(const double*, double*, const size_t, const size_t*)) {
  return guarded([&] {
    auto& in = top();
    in.apply_on_p_fort = func;
    ensure_r(in, buffer_size);
    upload(in, in.rp, buffer_size, parameters);
    upload(in, in.ra, buffer_size, action);
    std::vector<SparseP> pvectors(nP);
    for (size_t p = 0; p < nP; ++p)
      for (size_t k = offsets[p]; k < offsets[p + 1]; ++k) pvectors[p].emplace(indices[k], coefficients[k]);
    const size_t npp = (in.solver->dimensions().oP + nP) * nP;  // reference IterativeSolverCMPI.cpp:417
    std::vector<double> ppm(pp, pp + npp);
    Instance* ip = &in;
    // reference apply_on_p_c (IterativeSolverCMPI.cpp:141-157): the caller's routine adds the
    // P-space contributions to this rank's range of the action vectors, laid out as host arrays.
    auto apply = [ip](const std::vector<std::vector<double>>& pvecs, const it::CVecRef<SparseP>&,
                      const it::VecRef<Vec>& act) {
      Instance& I = *ip;
      const size_t nu = pvecs.size();
      std::vector<double> flat;
      for (const auto& v : pvecs) flat.insert(flat.end(), v.begin(), v.end());
      std::vector<size_t> ranges;
      for (size_t k = 0; k < nu; ++k) {
        ranges.push_back(I.offset);
        ranges.push_back(I.offset + I.local);
      }
      std::vector<double> host(nu * I.dimension, 0.0);
      for (size_t k = 0; k < nu; ++k)
        check(ssp_download(I.dev->ctx(), host.data() + k * I.dimension + I.offset, act[k].get().data(), I.local),
              "ssp_download");
      I.apply_on_p_fort(flat.data(), host.data() + I.offset, nu, ranges.data());
      for (size_t k = 0; k < nu; ++k)
        check(ssp_upload(I.dev->ctx(), act[k].get().data_wo(), host.data() + k * I.dimension + I.offset, I.local),
              "ssp_upload");
    };
    const RefineScratch scratch(in, parameters, action, in.dimension, false, buffer_size);
    const size_t nwork =
        in.solver->add_p(it::cwrap(pvectors), ppm, first(in.rp, buffer_size), first(in.ra, buffer_size), apply);
    download(in, in.rp, buffer_size, parameters);
    download(in, in.ra, buffer_size, action);
    if (sync) {
      synchronize(in, std::min(nwork, buffer_size), parameters);
      synchronize(in, std::min(nwork, buffer_size), action);
    }
    return nwork;
  });
}

// ---- R vectors in device memory (include/iterative_solver_c.h): each call is its host twin with the
// upload / download pairs replaced by import_rows / export_rows on this rank's shard.
size_t IterativeSolverHbmAddVectorDevice(size_t buffer_size, double* parameters, double* action, size_t ld) {
  return guarded([&] {
    auto& in = top();
    check_pair(in, buffer_size, parameters, action, ld, "IterativeSolverHbmAddVectorDevice");
    ensure_r(in, buffer_size);
    import_rows(in, in.rp, buffer_size, parameters, ld);
    import_rows(in, in.ra, buffer_size, action, ld);
    const RefineScratch scratch(in, parameters, action, ld, true, buffer_size);
    const size_t nwork = add_vector_staged(in, buffer_size);
    export_rows(in, in.rp, buffer_size, parameters, ld);
    export_rows(in, in.ra, buffer_size, action, ld);
    return nwork;
  });
}

void IterativeSolverHbmSolutionDevice(int nroot, int* roots, double* parameters, double* action, size_t ld) {
  guarded([&] {
    auto& in = top();
    const size_t n = size_t(nroot);
    check_pair(in, n, parameters, action, ld, "IterativeSolverHbmSolutionDevice");
    ensure_r(in, n);
    std::vector<int> r(roots, roots + nroot);
    in.solver->solution(r, first(in.rp, n), first(in.ra, n));
    export_rows(in, in.rp, n, parameters, ld);
    export_rows(in, in.ra, n, action, ld);
  });
}

size_t IterativeSolverHbmAddValueDevice(double value, double* parameters, double* action) {
  return guarded([&]() -> size_t {
    auto& in = top();
    check_pair(in, 1, parameters, action, in.local, "IterativeSolverHbmAddValueDevice");
    ensure_r(in, 1);
    import_rows(in, in.rp, 1, parameters, in.local);
    import_rows(in, in.ra, 1, action, in.local);
    const int r = in.solver->add_vector(in.rp[0], in.ra[0], value);
    export_rows(in, in.rp, 1, parameters, in.local);
    export_rows(in, in.ra, 1, action, in.local);
    return r > 0 ? 1 : 0;
  });
}

size_t IterativeSolverHbmEndIterationDevice(size_t buffer_size, double* solution, double* residual, size_t ld) {
  return guarded([&] {
    auto& in = top();
    check_pair(in, buffer_size, solution, residual, ld, "IterativeSolverHbmEndIterationDevice");
    ensure_r(in, buffer_size);
    import_rows(in, in.rp, buffer_size, solution, ld);
    import_rows(in, in.ra, buffer_size, residual, ld);
    const RefineScratch scratch(in, solution, residual, ld, true, buffer_size);  // a D-space rebuild's
    const size_t result = in.solver->end_iteration(first(in.rp, buffer_size), first(in.ra, buffer_size));
    // refined mode over an f32 Q space: the new parameter rows leave rounded, by the export itself where the
    // library has the export that rounds, else by a pass over the staging vectors first (the same bits)
    size_t mq = rounds_new_parameters(in) ? std::min(result, buffer_size) : 0;
    if (mq > 0 && !rows_export_q_fn) {
      in.solver->quantise(first(in.rp, mq));
      mq = 0;
    }
    export_rows(in, in.rp, buffer_size, solution, ld, mq);
    export_rows(in, in.ra, buffer_size, residual, ld);
    return result;
  });
}

void IterativeSolverHbmSetDiagonalsDevice(const double* diagonals) {
  guarded([&] {
    auto& in = top();
    check_rows(in, 1, diagonals, in.local, rows_import_fn != nullptr, "IterativeSolverHbmSetDiagonalsDevice");
    std::vector<Vec> d;
    d.emplace_back(in.dev, in.dimension);
    import_rows(in, d, 1, diagonals, in.local);
    in.diagonals = std::make_unique<Vec>(std::move(d[0]));
    store_diagonals_as_q(in);
  });
}

void IterativeSolverHbmDiagonalsDevice(double* diagonals) {
  guarded([&] {
    auto& in = top();
    if (!in.diagonals) throw std::runtime_error("IterativeSolverHbmDiagonalsDevice: no diagonals set");
    check_rows(in, 1, diagonals, in.local, rows_export_fn != nullptr, "IterativeSolverHbmDiagonalsDevice");
    std::vector<Vec> d{*in.diagonals};  // shares the storage
    export_rows(in, d, 1, diagonals, in.local);
  });
}

void IterativeSolverErrors(double* errors) {
  guarded([&] {
    size_t k = 0;
    for (double e : top().solver->errors()) errors[k++] = e;
  });
}

void IterativeSolverEigenvalues(double* eigenvalues) {
  guarded([&] {
    std::vector<double> ev;
    if (!top().solver->eigenvalues(ev)) return;
    std::copy(ev.begin(), ev.end(), eigenvalues);
  });
}

void IterativeSolverWorkingSetEigenvalues(double* eigenvalues) {
  guarded([&] {
    std::vector<double> ev;
    if (!top().solver->working_set_eigenvalues(ev)) return;
    std::copy(ev.begin(), ev.end(), eigenvalues);
  });
}

// reference IterativeSolverTemplate::suggest_p (IterativeSolverTemplate.h:238-241) returns no indices.
size_t IterativeSolverSuggestP(const double*, const double*, size_t, double, size_t*) { return 0; }

void IterativeSolverPrintStatistics(void) {
  guarded([] { std::cout << top().solver->statistics() << std::endl; });
}

int IterativeSolverNonLinear(void) {
  return guarded([] { return top().solver->nonlinear() ? 1 : 0; });
}
int IterativeSolverHasValues(void) {
  return guarded([] { return top().has_values ? 1 : 0; });
}
int IterativeSolverHasEigenvalues(void) {
  return guarded([] { return top().has_eigenvalues ? 1 : 0; });
}

void IterativeSolverSetDiagonals(const double* diagonals) {
  guarded([&] {
    auto& in = top();
    in.diagonals = std::make_unique<Vec>(in.dev, in.dimension);
    check(ssp_upload(in.dev->ctx(), in.diagonals->data_wo(), diagonals + in.offset, in.local), "ssp_upload");
    store_diagonals_as_q(in);
  });
}

void IterativeSolverDiagonals(double* diagonals) {
  guarded([&] {
    auto& in = top();
    if (!in.diagonals) throw std::runtime_error("IterativeSolverDiagonals: no diagonals set");
    check(ssp_download(in.dev->ctx(), diagonals + in.offset, in.diagonals->data(), in.local), "ssp_download");
  });
}

// reference IterativeSolverTemplate::value (IterativeSolverTemplate.h:312-315): NaN unless the
// subspace carries a value block (Optimize only).
double IterativeSolverValue(void) {
  return guarded([] { return top().solver->value(); });
}

int IterativeSolverVerbosity(void) {
  return guarded([] {
    switch (top().solver->get_verbosity()) {
      case it::Verbosity::None: return 0;
      case it::Verbosity::Summary: return 1;
      case it::Verbosity::Iteration: return 2;
      case it::Verbosity::Detailed: return 3;
    }
    return -1;
  });
}

int IterativeSolverMaxIter(void) {
  return guarded([] { return top().solver->get_max_iter(); });
}
void IterativeSolverSetMaxIter(int max_iter) {
  guarded([&] { top().solver->set_max_iter(max_iter); });
}

size_t IterativeSolverHbmNRoots(void) {
  return instances.empty() ? 0 : instances.back()->solver->n_roots();
}

// reference IterativeSolverCMPI.cpp:481-534 (mpi::comm_global / comm_self / size_global /
// rank_global / init / finalize), through the caller's MPI library when the process has one
// (mpi_bridge.h).  Without MPI the handles are 0 and size and rank are those of the context the next
// instance will use.  init calls MPI_Init when MPI is loaded but not initialised, and finalize undoes
// only that; both return 0 (MPI_SUCCESS) without MPI.  The reference's Fortran module binds the
// size/rank functions as IterativeSolver_mpi_size_global / _mpi_rank_global (IterativeSolverF.F90:50-57)
// while its C++ defines IterativeSolver_mpisize_global / _mpirank_global: both spellings exist here.
int64_t IterativeSolver_mpicomm_global(void) { return active_mpi() ? active_mpi()->world() : 0; }
int64_t IterativeSolver_mpicomm_self(void) { return active_mpi() ? active_mpi()->self() : 0; }
int64_t mpicomm_global(void) { return IterativeSolver_mpicomm_global(); }
int64_t mpicomm_self(void) { return IterativeSolver_mpicomm_self(); }
int64_t IterativeSolver_mpisize_global(void) {
  if (g_user_ctx) return ssp_ctx_nranks(g_user_ctx);
  auto* b = active_mpi();
  return b ? b->size(b->world()) : 1;
}
int64_t IterativeSolver_mpirank_global(void) {
  if (g_user_ctx) return ssp_ctx_rank(g_user_ctx);
  auto* b = active_mpi();
  return b ? b->rank(b->world()) : 0;
}
int64_t IterativeSolver_mpi_size_global(void) { return IterativeSolver_mpisize_global(); }
int64_t IterativeSolver_mpi_rank_global(void) { return IterativeSolver_mpirank_global(); }
int IterativeSolver_mpi_init(void) {
  auto* b = molpro::linalg::hbm::mpi::bridge();
  return b ? b->init() : 0;
}
int IterativeSolver_mpi_finalize(void) {
  auto* b = molpro::linalg::hbm::mpi::bridge();
  return b ? b->finalize() : 0;
}

int IterativeSolverHbmMpiActive(void) { return active_mpi() ? 1 : 0; }

// ---- the refined mode and the Q storage of the top instance (include/iterative_solver_c.h) ----------------
int IterativeSolverHbmSetRefineAction(itsolv_refine_action_fn fn, void* user) {
  return guarded([&] {
    auto& in = top();
    in.refine_fn = fn;
    in.refine_user = user;
    Instance* ip = &in;  // heap-held (instances)
    if (fn) in.solver->set_refine_action([ip](const it::CVecRef<Vec>& x, const it::VecRef<Vec>& a) { refine_action(*ip, x, a); });
    else in.solver->set_refine_action({});
    return 0;
  }) == 0 && g_error.empty() ? 0 : 1;
}

int IterativeSolverHbmRefineStatistics(int* refined_actions, int* first_refined_iteration, double* max_delta) {
  if (instances.empty()) return 1;
  const auto s = instances.back()->solver->refine_stats();
  if (refined_actions) *refined_actions = s.refined_actions;
  if (first_refined_iteration) *first_refined_iteration = s.first_refined_iteration;
  if (max_delta) *max_delta = s.max_delta;
  return 0;
}

int IterativeSolverHbmRefineDspaceStats(int* rebuilds, int* actions) {
  if (instances.empty()) return 1;
  const auto s = instances.back()->solver->refine_stats();
  if (rebuilds) *rebuilds = s.dspace_rebuilds;
  if (actions) *actions = s.dspace_actions;
  return 0;
}

size_t IterativeSolverHbmQStorage(void) { return instances.empty() ? 0 : instances.back()->solver->q_bytes(); }

size_t IterativeSolverHbmQuantise(size_t buffer_size, double* parameters) {
  return guarded([&]() -> size_t {
    auto& in = top();
    if (in.solver->q_bytes() >= sizeof(double) || buffer_size == 0) return 0;
    ensure_r(in, buffer_size);
    upload(in, in.rp, buffer_size, parameters);
    in.solver->quantise(first(in.rp, buffer_size));
    download(in, in.rp, buffer_size, parameters);
    return buffer_size;
  });
}

size_t IterativeSolverHbmQuantiseDevice(size_t buffer_size, double* parameters, size_t ld) {
  return guarded([&]() -> size_t {
    auto& in = top();
    if (in.solver->q_bytes() >= sizeof(double) || buffer_size == 0) return 0;
    const bool have = rows_import_fn && rows_export_fn;
    check_rows(in, buffer_size, parameters, ld, have, "IterativeSolverHbmQuantiseDevice");
    ensure_r(in, buffer_size);
    import_rows(in, in.rp, buffer_size, parameters, ld);
    if (rows_export_q_fn) {
      export_rows(in, in.rp, buffer_size, parameters, ld, buffer_size);
    } else {
      in.solver->quantise(first(in.rp, buffer_size));
      export_rows(in, in.rp, buffer_size, parameters, ld);
    }
    return buffer_size;
  });
}

int IterativeSolverHbmMpiAttach(ssp_ctx* ctx, int64_t fcomm, const char* transport) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("IterativeSolverHbmMpiAttach: null context");
    auto link = molpro::linalg::hbm::mpi::attach(ctx, fcomm, transport);
    // The caller owns ctx and detaches it by destroying it; the transport's callback state stays
    // with the process (a few bytes per attach).
    static std::vector<std::shared_ptr<void>> keep;
    if (link) keep.push_back(std::move(link));
    return 0;
  }) == 0 && g_error.empty() ? 0 : 1;
}

}  // extern "C"
