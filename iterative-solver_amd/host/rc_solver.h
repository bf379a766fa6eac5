// The Q-independent face of a solver behind the reverse-communication C API (iterative_solver_c.cpp).
//
// Everything the C layer calls on a solver takes R and P arguments only, so the instance holds this
// interface instead of IterativeSolverTemplate<Vec, Vec, SparseP>: RcSolverOf<Q> implements it over a solver
// with any Q.  Q = Vec is instantiated in host/; Q = VecF32 (Q_STORAGE=f32) in host_q32/, which host/ reaches
// through the weak make_rc_davidson_q32 below -- null where host/ is linked without host_q32/ (the CPU
// emulation of the f64 C ABI, which has no mixed-precision entry points).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "itsolv_hbm/hbm_handlers.h"
#include "itsolv_hbm/solvers.h"

namespace itsolv_rc {

namespace it = molpro::linalg::itsolv;
using molpro::linalg::hbm::SparseP;
using molpro::linalg::hbm::Vec;

class RcSolver {
 public:
  using fapply_on_p_type =
      std::function<void(const std::vector<std::vector<double>>&, const it::CVecRef<SparseP>&, const it::VecRef<Vec>&)>;
  using action_hook_type = std::function<void(const it::CVecRef<Vec>&, const it::VecRef<Vec>&)>;

  virtual ~RcSolver() = default;
  virtual bool nonlinear() const = 0;
  virtual int add_vector(const it::VecRef<Vec>& parameters, const it::VecRef<Vec>& actions) = 0;
  virtual int add_vector(Vec& parameters, Vec& actions, double value) = 0;
  virtual size_t add_p(const it::CVecRef<SparseP>& pparams, const std::vector<double>& pp, const it::VecRef<Vec>& parameters,
                       const it::VecRef<Vec>& actions, fapply_on_p_type apply_p) = 0;
  virtual void solution(const std::vector<int>& roots, const it::VecRef<Vec>& parameters, const it::VecRef<Vec>& residual) = 0;
  virtual size_t end_iteration(const it::VecRef<Vec>& parameters, const it::VecRef<Vec>& actions) = 0;
  virtual bool end_iteration_needed() const = 0;
  virtual const std::vector<int>& working_set() const = 0;
  virtual size_t n_roots() const = 0;
  virtual const std::vector<double>& errors() const = 0;
  virtual const it::Statistics& statistics() const = 0;
  virtual const it::subspace::Dimensions& dimensions() const = 0;
  virtual double value() const = 0;
  virtual void set_verbosity(it::Verbosity v) = 0;
  virtual void set_convergence_threshold(double t) = 0;
  virtual void set_convergence_threshold_value(double t) = 0;
  virtual it::Verbosity get_verbosity() const = 0;
  virtual int get_max_iter() const = 0;
  virtual void set_max_iter(int n) = 0;
  //! false for a solver without eigenvalues (nothing is written then)
  virtual bool eigenvalues(std::vector<double>& out) const = 0;
  virtual bool working_set_eigenvalues(std::vector<double>& out) const = 0;
  // refined mode (itsolv_hbm/refine.h)
  //! also checks the mode's scope (errors name the option)
  virtual void set_refine(const it::RefineOptions& o) = 0;
  virtual it::RefineOptions refine_options() const = 0;
  virtual void set_refine_action(action_hook_type hook) = 0;
  virtual it::RefineStats refine_stats() const = 0;
  //! bytes per stored Q element
  virtual size_t q_bytes() const = 0;
  //! rounds the vectors to the Q storage format in place (nothing for a Q space stored as R)
  virtual void quantise(const it::VecRef<Vec>& xx) = 0;
};

template <class Q>
class RcSolverOf final : public RcSolver {
  using Solver = it::IterativeSolverTemplate<Vec, Q, SparseP>;
  using Davidson = it::DavidsonSolver<Vec, Q, SparseP>;
  using Handlers = std::shared_ptr<it::ArrayHandlers<Vec, Q, SparseP>>;

 public:
  RcSolverOf(std::unique_ptr<Solver> solver, Handlers handlers, size_t q_bytes = sizeof(double))
      : m_s(std::move(solver)),
        m_davidson(dynamic_cast<Davidson*>(m_s.get())),
        m_h(std::move(handlers)),
        m_q_bytes(q_bytes) {}

  bool nonlinear() const override { return m_s->nonlinear(); }
  int add_vector(const it::VecRef<Vec>& p, const it::VecRef<Vec>& a) override { return m_s->add_vector(p, a); }
  int add_vector(Vec& p, Vec& a, double value) override { return m_s->add_vector(p, a, value); }
  size_t add_p(const it::CVecRef<SparseP>& pparams, const std::vector<double>& pp, const it::VecRef<Vec>& p,
               const it::VecRef<Vec>& a, fapply_on_p_type apply_p) override {
    return m_s->add_p(pparams, pp, p, a, std::move(apply_p));
  }
  void solution(const std::vector<int>& roots, const it::VecRef<Vec>& p, const it::VecRef<Vec>& r) override {
    m_s->solution(roots, p, r);
  }
  size_t end_iteration(const it::VecRef<Vec>& p, const it::VecRef<Vec>& a) override { return m_s->end_iteration(p, a); }
  bool end_iteration_needed() const override { return m_s->end_iteration_needed(); }
  const std::vector<int>& working_set() const override { return m_s->working_set(); }
  size_t n_roots() const override { return m_s->n_roots(); }
  const std::vector<double>& errors() const override { return m_s->errors(); }
  const it::Statistics& statistics() const override { return m_s->statistics(); }
  const it::subspace::Dimensions& dimensions() const override { return m_s->dimensions(); }
  double value() const override { return m_s->value(); }
  void set_verbosity(it::Verbosity v) override { m_s->set_verbosity(v); }
  void set_convergence_threshold(double t) override { m_s->set_convergence_threshold(t); }
  void set_convergence_threshold_value(double t) override { m_s->set_convergence_threshold_value(t); }
  it::Verbosity get_verbosity() const override { return m_s->get_verbosity(); }
  int get_max_iter() const override { return m_s->get_max_iter(); }
  void set_max_iter(int n) override { m_s->set_max_iter(n); }
  bool eigenvalues(std::vector<double>& out) const override {
    if (auto* d = dynamic_cast<const it::LinearEigensystemDavidson<Vec, Q, SparseP>*>(m_s.get())) out = d->eigenvalues();
    else if (auto* r = dynamic_cast<const it::LinearEigensystemRSPT<Vec, Q, SparseP>*>(m_s.get())) out = r->eigenvalues();
    else return false;
    return true;
  }
  bool working_set_eigenvalues(std::vector<double>& out) const override {
    if (!dynamic_cast<const it::LinearEigensystemDavidson<Vec, Q, SparseP>*>(m_s.get()) &&
        !dynamic_cast<const it::LinearEigensystemRSPT<Vec, Q, SparseP>*>(m_s.get()))
      return false;
    out = m_s->working_set_eigenvalues();
    return true;
  }
  void set_refine(const it::RefineOptions& o) override {
    if (!m_davidson && o.on)
      throw std::logic_error("refine: available for the hermitian LinearEigensystemDavidson and LinearEquationsDavidson only");
    if (!m_davidson) return;
    if (o.on && !o.dspace) m_davidson->validate_refine();
    m_davidson->set_refine(o.on, o.kappa);
    if (o.on && o.dspace) {  // the scope depends on the option: checked with it set
      m_davidson->set_refine_dspace(true);
      m_davidson->validate_refine();
      m_davidson->set_refine_dspace_slack(o.dspace_slack);
    }
  }
  it::RefineOptions refine_options() const override {
    return m_davidson ? m_davidson->refine_options() : it::RefineOptions{};
  }
  void set_refine_action(action_hook_type hook) override {
    if (m_davidson) m_davidson->set_refine_action(std::move(hook));
  }
  it::RefineStats refine_stats() const override { return m_davidson ? m_davidson->refine_stats() : it::RefineStats{}; }
  size_t q_bytes() const override { return m_q_bytes; }
  void quantise(const it::VecRef<Vec>& xx) override {
    using molpro::linalg::array::quantise_for_storage;
    quantise_for_storage(m_h->qr(), xx);
  }

  Solver& solver() { return *m_s; }

 private:
  std::unique_ptr<Solver> m_s;
  Davidson* m_davidson;  // m_s where it is one, else null
  Handlers m_h;
  size_t m_q_bytes;
};

// The hermitian-or-not LinearEigensystem "Davidson" over make_handlers_q32() (host_q32/rc_q32.cpp), options
// parsed as create_LinearEigensystem parses them.  Weak: null without host_q32/.
std::unique_ptr<RcSolver> make_rc_davidson_q32(const std::string& options, size_t nroot, bool hermitian)
    __attribute__((weak));
// LinearEquations "Davidson" over the same handlers, for the right-hand sides rhs (R vectors), set up as
// IterativeSolverLinearEquationsInitialize sets up the f64 solver.  refine.on: the refined mode, set before the
// equations are added (it keeps their twins in R's format) and its scope checked once everything is set (errors
// name the option); off: the plain f32 Q space.  Weak: null without host_q32/.
std::unique_ptr<RcSolver> make_rc_linear_equations_q32(const std::string& options, std::vector<Vec>& rhs, bool hermitian,
                                                       double augmented_hessian, const it::RefineOptions& refine)
    __attribute__((weak));
// NonLinearEquations "DIIS" over the same handlers with its history stored as f32 differences behind f64 anchors
// (itsolv_hbm/diis_differences.h: NonLinearEquationsDIISDifferences<Vec, VecF32, SparseP>), options parsed as
// create_NonLinearEquations parses them.  Weak: null without host_q32/.
std::unique_ptr<RcSolver> make_rc_diis_q32(const std::string& options) __attribute__((weak));

}  // namespace itsolv_rc
