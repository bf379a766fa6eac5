// Q_STORAGE=f32 of the reverse-communication C API (include/iterative_solver_c.h): the instance's solver as
// LinearEigensystemDavidson<Vec, VecF32, SparseP>, LinearEquationsDavidson<Vec, VecF32, SparseP> or
// NonLinearEquationsDIISDifferences<Vec, VecF32, SparseP> over make_handlers_q32(), behind the Q-independent face of host/rc_solver.h.  It lives here, not in host/, for the reason host_q32/itsolv_q32.cpp does: the handlers
// call the mixed-precision C ABI, which the CPU emulation that host/ is also linked against does not have.
#include "../host/rc_solver.h"
#include "itsolv_hbm/diis_differences.h"
#include "itsolv_hbm/hbm_handlers_f32.h"
#include "itsolv_hbm/solver_factory.h"

namespace itsolv_rc {

std::unique_ptr<RcSolver> make_rc_davidson_q32(const std::string& options, size_t nroot, bool hermitian) {
  using molpro::linalg::hbm::VecF32;
  auto handlers = molpro::linalg::hbm::make_handlers_q32();
  auto solver = it::create_LinearEigensystem("Davidson", options, handlers);
  solver->set_n_roots(nroot);
  if (auto* d = dynamic_cast<it::LinearEigensystemDavidson<Vec, VecF32, SparseP>*>(solver.get()))
    d->set_hermiticity(hermitian);
  return std::make_unique<RcSolverOf<VecF32>>(std::move(solver), std::move(handlers), sizeof(float));
}

std::unique_ptr<RcSolver> make_rc_linear_equations_q32(const std::string& options, std::vector<Vec>& rhs, bool hermitian,
                                                       double augmented_hessian, const it::RefineOptions& refine) {
  using molpro::linalg::hbm::VecF32;
  using LinEq = it::LinearEquationsDavidson<Vec, VecF32, SparseP>;
  auto handlers = molpro::linalg::hbm::make_handlers_q32();
  auto solver = it::create_LinearEquations("Davidson", options, handlers);
  auto* s = dynamic_cast<LinEq*>(solver.get());
  if (!s) throw std::logic_error("Q_STORAGE=f32: LinearEquations is not the Davidson solver");
  if (refine.on) s->set_refine(true, refine.kappa);  // before the equations: their twins are kept from here on
  s->set_hermiticity(hermitian);
  s->set_n_roots(rhs.size());
  s->add_equations(rhs);
  if (augmented_hessian > 0) s->set_augmented_hessian(augmented_hessian);
  if (refine.on) s->validate_refine();
  return std::make_unique<RcSolverOf<VecF32>>(std::move(solver), std::move(handlers), sizeof(float));
}

std::unique_ptr<RcSolver> make_rc_diis_q32(const std::string& options) {
  using molpro::linalg::hbm::VecF32;
  auto handlers = molpro::linalg::hbm::make_handlers_q32();
  auto solver = std::make_unique<it::NonLinearEquationsDIISDifferences<Vec, VecF32, SparseP>>(handlers);
  solver->set_options(it::NonLinearEquationsDIISOptions{it::parse_options(options)});  // create_NonLinearEquations'
  return std::make_unique<RcSolverOf<VecF32>>(std::move(solver), std::move(handlers), sizeof(float));
}

}  // namespace itsolv_rc
