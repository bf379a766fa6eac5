// DIIS over a history stored as differences on the CPU (itsolv_hbm/diis_differences.h): the C5 problem form of
// itsolv_hbm/problems.h c5_spec -- r = H (x - t 1), H = diag(1 + 2 frac(g phi1)) + (1/n) 1 1^T, the
// preconditioner's diagonal mismatched by alpha = 0.2, t = 1/sqrt(n), from x = e_0 -- on the minimal double / float
// handlers of tests/cpp/rc_model_handlers.h.  No device: what runs is the solver's call-by-call sequence (the
// differences stored by copy, axpy(-1), narrowing copy; the new row of H from one overlap with the stored
// differences; the anchor's copy and one gemm_outer per construction; the merging axpy of a deletion).
//
//   q32_diis_model <n> <threshold> <max_iter> <mode> <max_size_qspace, 0: none> <middle: 0 | 1 | 2>
// mode: points64 (NonLinearEquationsDIIS, Q as double), points32 (the same, Q as float), diff64
// (NonLinearEquationsDIISDifferences, Q as double: the control), diff32 (Q as float), or refuse_p (diff32 with
// max_p = 4: prints {"error": <the message>}).
// middle = 1: after every iteration that leaves 5 or more points and is not converged, point 2 is deleted -- neither
// the newest nor the oldest -- in the point form through xspace().eraseq and in the difference form through
// erase_point.
// middle = 2 (the difference form only): point 0 of two or more is deleted after the second iteration, which the
// solver refuses: prints {"error": <the message>}.
// Prints one JSON line: converged, iterations, errors (the solver's, one per iteration), best_error, true_residual
// (|H (x - t 1)| recomputed here in double from the solver's final parameters), points, pairs, anchors, merged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rc_model_handlers.h"

#include "itsolv_hbm/diis_differences.h"
#include "itsolv_hbm/problems.h"

namespace model {

namespace it = molpro::linalg::itsolv;

struct C5Problem : it::Problem<Arr<double>, SP> {
  using R = Arr<double>;
  it::problems::SyntheticSpec s;
  explicit C5Problem(size_t n) : s(it::problems::c5_spec(n)) {}
  // r = H (x - t 1): the diagonal part, then rho <1, x - t 1> on every element
  double residual(const R& x, R& r) const override {
    double sum = 0;
    for (size_t g = 0; g < s.n; ++g) sum += x.v[g] - s.target;
    for (size_t g = 0; g < s.n; ++g) r.v[g] = s.d(g) * (x.v[g] - s.target) + s.rho * sum;
    return 0;
  }
  bool diagonals(R& d) const override {
    for (size_t g = 0; g < s.n; ++g) d.v[g] = s.diagonal(g);
    return true;
  }
  // (refuse_p: solve() asks for this before it reaches the solver's add_p)
  std::vector<double> pp_action_matrix(const std::vector<SP>& pp) const override {
    std::vector<double> m;
    for (auto& a : pp)
      for (auto& b : pp) m.push_back(s.h(a.begin()->first, b.begin()->first));
    return m;
  }
};

std::string list(const std::vector<double>& v) {
  std::string s = "[";
  char buf[40];
  for (size_t i = 0; i < v.size(); ++i) {
    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]);
    s += buf;
  }
  return s + "]";
}

template <class T>
struct is_differences : std::false_type {};
template <class R, class Q, class P>
struct is_differences<it::NonLinearEquationsDIISDifferences<R, Q, P>> : std::true_type {};

template <class Solver, class SQ>
int run(size_t n, double threshold, int max_iter, int max_size_qspace, int middle, int max_p) {
  using R = Arr<double>;
  const C5Problem problem(n);
  Solver solver(handlers<SQ>());
  it::NonLinearEquationsDIISOptions opt;
  opt.n_roots = 1;
  opt.convergence_threshold = threshold;
  opt.max_iter = max_iter;
  opt.max_p = max_p;
  opt.verbosity = it::Verbosity::None;
  if (max_size_qspace > 0) opt.max_size_qspace = max_size_qspace;
  solver.set_options(opt);
  R x(n), r(n);
  x.v[0] = 1;
  std::vector<double> errors;
  size_t points = 0;
  solver.iteration_hook = [&] {
    const double e = solver.errors().empty() ? 0.0 : solver.errors().front();
    errors.push_back(e);
    points = solver.dimensions().nQ;
    if constexpr (is_differences<Solver>::value)
      if (middle == 2 && points >= 2) solver.erase_point(0);
    if (middle == 1 && points >= 5 && e >= threshold) {
      if constexpr (is_differences<Solver>::value) solver.erase_point(2);
      else solver.xspace().eraseq(2);
    }
  };
  const bool converged = solver.solve(x, r, problem);
  // the solver's final parameters (the anchor when converged), and their residual recomputed here
  R xs(n), rs(n);
  double best = errors.empty() ? 0.0 : errors.front();
  for (double e : errors) best = std::min(best, e);
  double true_residual = std::nan("");
  if (!middle || converged) {  // (a deletion after the last iteration leaves no subspace solution to construct from)
    solver.solution_params(std::vector<int>{0}, it::VecRef<R>{std::ref(xs)});
    problem.residual(xs, rs);
    double rr = 0;
    for (double e : rs.v) rr += e * e;
    true_residual = std::sqrt(rr);
  }
  size_t pairs = 0, anchors = 0, merged = 0;
  if constexpr (is_differences<Solver>::value) {
    pairs = solver.difference_pairs();
    anchors = solver.anchors();
    merged = solver.merged_deletions();
  }
  std::printf("{\"converged\": %s, \"iterations\": %d, \"errors\": %s, \"best_error\": %.17g, \"true_residual\": %.17g, "
              "\"points\": %zu, \"pairs\": %zu, \"anchors\": %zu, \"merged\": %zu}\n",
              converged ? "true" : "false", solver.statistics().iterations, list(errors).c_str(), best, true_residual,
              size_t(solver.dimensions().nQ), pairs, anchors, merged);
  return 0;
}

}  // namespace model

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s n threshold max_iter mode max_size_qspace middle\n", argv[0]);
    return 2;
  }
  using namespace model;
  using R = Arr<double>;
  const size_t n = size_t(std::atol(argv[1]));
  const double threshold = std::atof(argv[2]);
  const int max_iter = std::atoi(argv[3]);
  const std::string mode = argv[4];
  const int mq = std::atoi(argv[5]);
  const int middle = std::atoi(argv[6]);
  try {
    if (mode == "points64") return run<it::NonLinearEquationsDIIS<R, Arr<double>, SP>, double>(n, threshold, max_iter, mq, middle, 0);
    if (mode == "points32") return run<it::NonLinearEquationsDIIS<R, Arr<float>, SP>, float>(n, threshold, max_iter, mq, middle, 0);
    if (mode == "diff64")
      return run<it::NonLinearEquationsDIISDifferences<R, Arr<double>, SP>, double>(n, threshold, max_iter, mq, middle, 0);
    if (mode == "diff32")
      return run<it::NonLinearEquationsDIISDifferences<R, Arr<float>, SP>, float>(n, threshold, max_iter, mq, middle, 0);
    if (mode == "refuse_p")
      return run<it::NonLinearEquationsDIISDifferences<R, Arr<float>, SP>, float>(n, threshold, max_iter, mq, middle, 4);
  } catch (const std::exception& e) {
    std::string msg = e.what();
    for (auto& c : msg)
      if (c == '"' || c == '\\') c = '\'';
    std::printf("{\"error\": \"%s\"}\n", msg.c_str());
    return 0;
  }
  std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
