// The refined mode driven by hand, as the reverse-communication API drives it (no solve()): quantise, action,
// add_vector, precondition, end_iteration, with the refined residuals' action given by set_refine_action.
// LinearEigensystemDavidson<R over double, Q over float> on the minimal handler of rc_model_handlers.h; no device.
//
//   rc_refine_model <matrix file: n*n doubles, row-major> <n> <nroots> <threshold> <max_iter> <mode>
// mode: f64 (Q stored as double), q32 (Q stored as float, no set_refine), refined (Q as float, set_refine and
// set_refine_action), noaction (as refined, without set_refine_action: the error is printed, exit status 3).
// Prints the JSON line of tests/cpp/q32_refined_model.cpp.
#include <fstream>
#include <iostream>

#include "rc_model_handlers.h"

namespace model {

template <class SQ>
int run(const DenseProblem& problem, int nroots, double threshold, int max_iter, bool refine, bool give_action) {
  using R = Arr<double>;
  using Q = Arr<SQ>;
  using molpro::linalg::itsolv::cwrap;
  using molpro::linalg::itsolv::wrap;
  auto h = handlers<SQ>();
  molpro::linalg::itsolv::LinearEigensystemDavidson<R, Q, SP> solver(h);
  solver.set_n_roots(size_t(nroots));
  solver.set_convergence_threshold(threshold);
  solver.set_hermiticity(true);
  solver.set_verbosity(molpro::linalg::itsolv::Verbosity::None);
  if (refine) {
    solver.validate_refine();
    solver.set_refine(true);
    if (give_action) solver.set_refine_action([&problem](const CVecRef<R>& x, const VecRef<R>& a) { problem.action(x, a); });
  }
  std::vector<R> x, a;
  for (int i = 0; i < nroots; ++i) {
    x.emplace_back(problem.n);
    a.emplace_back(problem.n);
  }
  // solve()'s default guess: unit vectors on the nroots smallest diagonals, in index order
  R diag(problem.n);
  problem.diagonals(diag);
  {
    int root = 0;
    for (const auto& g : h->rr().select(size_t(nroots), diag)) x[size_t(root++)].v[g.first] = 1.0;
  }
  int nwork = nroots;
  for (int iter = 0; iter < max_iter && nwork > 0; ++iter) {
    if (refine) {  // what IterativeSolverEndIteration returns is rounded; the guess is the caller's to round
      using molpro::linalg::array::quantise_for_storage;
      quantise_for_storage(h->qr(), wrap(x.begin(), x.begin() + nwork));
    }
    problem.action(cwrap(x.begin(), x.begin() + nwork), wrap(a.begin(), a.begin() + nwork));
    nwork = solver.add_vector(x, a);
    while (solver.end_iteration_needed()) {
      if (nwork > 0) problem.precondition(wrap(a.begin(), a.begin() + nwork), solver.working_set_eigenvalues(), diag);
      nwork = int(solver.end_iteration(x, a));
    }
  }
  double emax = 0;
  for (double e : solver.errors()) emax = std::max(emax, e);
  const bool converged = nwork == 0 && emax <= threshold;
  const long solve_actions = problem.actions;
  const auto ev = solver.eigenvalues();
  std::vector<double> rn;
  for (int r = 0; r < nroots; ++r) {
    solver.solution(std::vector<int>{r}, x, a);
    R hx(problem.n);
    problem.apply(x[0], hx);
    double rr = 0, xx = 0;
    for (size_t i = 0; i < problem.n; ++i) {
      const double t = hx.v[i] - ev[size_t(r)] * x[0].v[i];
      rr += t * t;
      xx += x[0].v[i] * x[0].v[i];
    }
    rn.push_back(std::sqrt(rr / xx));
  }
  double max_delta = 0;
  for (double d : solver.refine_delta()) max_delta = std::max(max_delta, d);
  auto list = [](const std::vector<double>& v, size_t n) {
    std::string s = "[";
    char buf[40];
    for (size_t i = 0; i < n && i < v.size(); ++i) {
      std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]);
      s += buf;
    }
    return s + "]";
  };
  std::printf(
      "{\"converged\": %s, \"iterations\": %d, \"eigenvalues\": %s, \"errors\": %s, \"residual_norms\": %s, "
      "\"refined_actions\": %d, \"first_refined_iteration\": %d, \"max_delta\": %.17g, \"actions\": %ld}\n",
      converged ? "true" : "false", solver.statistics().iterations, list(ev, size_t(nroots)).c_str(),
      list(solver.errors(), size_t(nroots)).c_str(), list(rn, size_t(nroots)).c_str(), solver.refined_actions(),
      solver.first_refined_iteration(), max_delta, solve_actions);
  return 0;
}

}  // namespace model

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s matrix n nroots threshold max_iter f64|q32|refined|noaction\n", argv[0]);
    return 2;
  }
  model::DenseProblem problem;
  problem.n = size_t(std::atol(argv[2]));
  problem.h.resize(problem.n * problem.n);
  std::ifstream f(argv[1], std::ios::binary);
  f.read(reinterpret_cast<char*>(problem.h.data()), std::streamsize(problem.h.size() * sizeof(double)));
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  const int nroots = std::atoi(argv[3]), max_iter = std::atoi(argv[5]);
  const double threshold = std::atof(argv[4]);
  const std::string mode = argv[6];
  try {
    if (mode == "f64") return model::run<double>(problem, nroots, threshold, max_iter, false, false);
    if (mode == "q32") return model::run<float>(problem, nroots, threshold, max_iter, false, false);
    if (mode == "refined") return model::run<float>(problem, nroots, threshold, max_iter, true, true);
    if (mode == "noaction") return model::run<float>(problem, nroots, threshold, max_iter, true, false);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return mode == "noaction" ? 3 : 1;
  }
  std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
