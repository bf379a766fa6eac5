// Linear equations with the Q space in f32 on the CPU (itsolv_hbm/solvers.h LinearEquationsDavidson, plain and
// in the refined mode of set_refine): LinearEquationsDavidson<R, Q, P> with R over double storage and Q over
// float storage, on the minimal handlers of tests/cpp/q32_refined_model.cpp restated here.  No device: what runs
// is the solver's quantise-before-action call, the refined rows of subspace.h with the right-hand sides' twins
// (call by call), construct_residual against the twins, and the bound (scaled by 1 / |b|) and trigger of
// refine_residuals.
//
//   q32_lineq_model <matrix: n*n doubles> <n> <rhs: nrhs*n doubles> <nrhs> <threshold> <max_iter> <max_p> <mode>
//                   [<solutions out: nrhs*n doubles>]
// mode: f64 (Q stored as double), q32 (Q as float, plain), refined (Q as float, set_refine), or one of the
// refusals hermitian, max_size_qspace, reset_D, reset_D_max_Q_size, augmented_hessian, refine_dspace, late
// (set_refine after add_equations), which print {"error": <the message>}.
// Prints one JSON line: converged, iterations, errors, residual_norms (|A x - b| / |b| recomputed here), xnorm,
// bnorm, refined_actions, first_refined_iteration, max_delta, actions (all calls' vectors), nq (final Q size).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "itsolv_hbm/array_handlers.h"
#include "itsolv_hbm/solvers.h"
#include "itsolv_hbm/sparse_handler.h"

namespace model {

using molpro::linalg::array::ArrayHandler;
using molpro::linalg::itsolv::CVecRef;
using molpro::linalg::itsolv::VecRef;
using molpro::linalg::itsolv::subspace::Matrix;
using SP = std::map<size_t, double>;

// A vector whose logical element type is double and whose storage is S.
template <class S>
struct Arr {
  using value_type = double;
  using storage_type = S;
  std::vector<S> v;
  Arr() = default;
  explicit Arr(size_t n) : v(n, S(0)) {}
  size_t size() const { return v.size(); }
};

// Every operation in double, a result rounded once (nearest-even) where the destination stores float.
template <class SL, class SR>
class Handler : public ArrayHandler<Arr<SL>, Arr<SR>> {
  using AL = Arr<SL>;
  using AR = Arr<SR>;
  using Base = ArrayHandler<AL, AR>;

 public:
  using typename Base::ProxyHandle;
  using Base::lazy_handle;
  ProxyHandle lazy_handle() override { return this->lazy_handle(*this); }
  AL copy(const AR& s) override {
    AL x(s.size());
    copy(x, s);
    return x;
  }
  void copy(AL& x, const AR& y) override {
    x.v.resize(y.size());
    for (size_t i = 0; i < y.size(); ++i) x.v[i] = SL(y.v[i]);
  }
  void scal(double a, AL& x) override {
    for (auto& e : x.v) e = SL(a * double(e));
  }
  void fill(double a, AL& x) override {
    for (auto& e : x.v) e = SL(a);
  }
  void axpy(double a, const AR& x, AL& y) override {
    for (size_t i = 0; i < y.size(); ++i) y.v[i] = SL(double(y.v[i]) + a * double(x.v[i]));
  }
  double dot(const AL& x, const AR& y) override {
    double s = 0;
    for (size_t i = 0; i < x.size(); ++i) s += double(x.v[i]) * double(y.v[i]);
    return s;
  }
  void gemm_outer(const Matrix<double> al, const CVecRef<AR>& xx, const VecRef<AL>& yy) override {
    for (size_t i = 0; i < al.rows(); ++i)
      for (size_t j = 0; j < al.cols(); ++j) axpy(al(i, j), xx.at(i).get(), yy[j].get());
  }
  Matrix<double> gemm_inner(const CVecRef<AL>& xx, const CVecRef<AR>& yy) override {
    Matrix<double> m({xx.size(), yy.size()});
    for (size_t i = 0; i < m.rows(); ++i)
      for (size_t j = 0; j < m.cols(); ++j) m(i, j) = dot(xx.at(i).get(), yy.at(j).get());
    return m;
  }
  std::map<size_t, double> select_max_dot(size_t n, const AL& x, const AR& y) override {
    std::multimap<double, size_t, std::greater<double>> o;
    for (size_t i = 0; i < x.size(); ++i) o.emplace(std::abs(double(x.v[i]) * double(y.v[i])), i);
    std::map<size_t, double> out;
    for (auto it = o.begin(); it != o.end() && out.size() < n; ++it) out.emplace(it->second, it->first);
    return out;
  }
  std::map<size_t, double> select(size_t n, const AL& x, bool max = false, bool ignore_sign = false) override {
    std::multimap<double, size_t> o;
    for (size_t i = 0; i < x.size(); ++i) {
      const double e = ignore_sign ? std::abs(double(x.v[i])) : double(x.v[i]);
      o.emplace(max ? -e : e, i);
    }
    std::map<size_t, double> out;
    for (auto it = o.begin(); it != o.end() && out.size() < n; ++it) out.emplace(it->second, double(x.v[it->second]));
    return out;
  }
};

template <class S>
class SparseHandler : public ArrayHandler<Arr<S>, SP> {
  using A = Arr<S>;
  using Base = ArrayHandler<A, SP>;

 public:
  using typename Base::ProxyHandle;
  using Base::lazy_handle;
  ProxyHandle lazy_handle() override { return this->lazy_handle(*this); }
  A copy(const SP&) override { throw std::logic_error("no dense copy of a sparse vector"); }
  void copy(A& x, const SP& y) override {
    for (auto& e : x.v) e = S(0);
    for (auto& [i, c] : y) x.v.at(i) = S(c);
  }
  void scal(double, A&) override {}
  void fill(double, A&) override {}
  void axpy(double a, const SP& x, A& y) override {
    for (auto& [i, c] : x) y.v.at(i) = S(double(y.v[i]) + a * c);
  }
  double dot(const A& x, const SP& y) override {
    double s = 0;
    for (auto& [i, c] : y) s += double(x.v.at(i)) * c;
    return s;
  }
  void gemm_outer(const Matrix<double> al, const CVecRef<SP>& xx, const VecRef<A>& yy) override {
    for (size_t i = 0; i < al.rows(); ++i)
      for (size_t j = 0; j < al.cols(); ++j) axpy(al(i, j), xx.at(i).get(), yy[j].get());
  }
  Matrix<double> gemm_inner(const CVecRef<A>& xx, const CVecRef<SP>& yy) override {
    Matrix<double> m({xx.size(), yy.size()});
    for (size_t i = 0; i < m.rows(); ++i)
      for (size_t j = 0; j < m.cols(); ++j) m(i, j) = dot(xx.at(i).get(), yy.at(j).get());
    return m;
  }
  std::map<size_t, double> select_max_dot(size_t, const A&, const SP&) override { return {}; }
  std::map<size_t, double> select(size_t, const A&, bool = false, bool = false) override { return {}; }
};

// The hook of the refined mode for this file's vectors (found by argument-dependent lookup): R vectors
// rounded in place to the values Handler<float, double>::copy stores.
inline bool quantise_for_storage(ArrayHandler<Arr<float>, Arr<double>>&, const VecRef<Arr<double>>& xx) {
  for (auto& x : xx)
    for (auto& e : x.get().v) e = double(float(e));
  return true;
}

// Problem<R, P>'s default preconditioner for this file's R (the generic one wants an iterable container).
inline void precondition_default(const VecRef<Arr<double>>& r, const std::vector<double>& shift, const Arr<double>& d) {
  for (size_t k = 0; k < r.size(); ++k)
    for (size_t i = 0; i < d.size(); ++i) r[k].get().v[i] = r[k].get().v[i] / (d.v[i] - shift[k] + 1e-15);
}

template <class SQ>
auto handlers() {
  using R = Arr<double>;
  using Q = Arr<SQ>;
  return molpro::linalg::itsolv::ArrayHandlers<R, Q, SP>::create()
      .rr(std::make_shared<Handler<double, double>>())
      .qq(std::make_shared<Handler<SQ, SQ>>())
      .pp(std::make_shared<molpro::linalg::hbm::ArrayHandlerSparse>())
      .rq(std::make_shared<Handler<double, SQ>>())
      .rp(std::make_shared<SparseHandler<double>>())
      .qr(std::make_shared<Handler<SQ, double>>())
      .qp(std::make_shared<SparseHandler<SQ>>())
      .build_shared();
}

struct DenseProblem : molpro::linalg::itsolv::Problem<Arr<double>, SP> {
  using R = Arr<double>;
  std::vector<double> h;
  size_t n;
  mutable long actions = 0;
  void apply(const R& x, R& y) const {
    for (size_t i = 0; i < n; ++i) {
      const double* row = h.data() + i * n;
      double s[4] = {0, 0, 0, 0};
      size_t j = 0;
      for (; j + 4 <= n; j += 4)
        for (int e = 0; e < 4; ++e) s[e] += row[j + e] * x.v[j + e];
      double t = (s[0] + s[1]) + (s[2] + s[3]);
      for (; j < n; ++j) t += row[j] * x.v[j];
      y.v[i] = t;
    }
  }
  void action(const CVecRef<R>& x, const VecRef<R>& y) const override {
    for (size_t k = 0; k < x.size(); ++k) apply(x[k].get(), y[k].get());
    actions += long(x.size());
  }
  bool diagonals(R& d) const override {
    for (size_t i = 0; i < n; ++i) d.v[i] = h[i * n + i];
    return true;
  }
  std::vector<double> pp_action_matrix(const std::vector<SP>& pp) const override {
    std::vector<double> m;
    for (auto& a : pp)
      for (auto& b : pp) m.push_back(h[a.begin()->first * n + b.begin()->first]);
    return m;
  }
  void p_action(const std::vector<std::vector<double>>& c, const CVecRef<SP>& pp, const VecRef<R>& act) const override {
    for (size_t k = 0; k < c.size(); ++k)
      for (size_t p = 0; p < pp.size(); ++p)
        for (auto& [i, coef] : pp[p].get())
          for (size_t j = 0; j < n; ++j) act[k].get().v[j] += h[j * n + i] * coef * c[k][p];
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

template <class SQ>
int run(const DenseProblem& problem, const std::vector<Arr<double>>& rhs, double threshold, int max_iter, int max_p,
        const std::string& mode, const char* solutions_out) {
  using R = Arr<double>;
  using Q = Arr<SQ>;
  namespace it = molpro::linalg::itsolv;
  it::LinearEquationsDavidson<R, Q, SP> solver(handlers<SQ>());
  const bool refine = mode != "f64" && mode != "q32";
  if (refine && mode != "late") solver.set_refine(true);
  solver.add_equations(rhs);
  if (mode == "late") solver.set_refine(true);  // throws: the twins cannot be rebuilt
  solver.set_convergence_threshold(threshold);
  solver.set_max_iter(max_iter);
  solver.set_max_p(max_p);
  solver.set_verbosity(it::Verbosity::None);
  if (mode == "hermitian") solver.set_hermiticity(false);
  if (mode == "max_size_qspace") solver.set_max_size_qspace(30);
  if (mode == "reset_D") solver.set_reset_D(5);
  if (mode == "reset_D_max_Q_size") solver.set_reset_D_maxQ_size(30);
  if (mode == "augmented_hessian") solver.set_augmented_hessian(0.5);
  if (mode == "refine_dspace") solver.set_refine_dspace(true);
  const size_t nrhs = rhs.size();
  std::vector<R> x, a;
  for (size_t i = 0; i < nrhs; ++i) {
    x.emplace_back(problem.n);
    a.emplace_back(problem.n);
  }
  const bool converged = solver.solve(x, a, problem, true);
  const long solve_actions = problem.actions;
  std::vector<double> rn, xn, bn;
  std::vector<double> all;
  for (size_t r = 0; r < nrhs; ++r) {
    solver.solution(std::vector<int>{int(r)}, x, a);
    R hx(problem.n);
    problem.apply(x[0], hx);
    double rr = 0, xx = 0, bb = 0;
    for (size_t i = 0; i < problem.n; ++i) {
      const double t = hx.v[i] - rhs[r].v[i];
      rr += t * t;
      xx += x[0].v[i] * x[0].v[i];
      bb += rhs[r].v[i] * rhs[r].v[i];
    }
    rn.push_back(std::sqrt(rr / bb));
    xn.push_back(std::sqrt(xx));
    bn.push_back(std::sqrt(bb));
    all.insert(all.end(), x[0].v.begin(), x[0].v.end());
  }
  if (solutions_out) {
    std::ofstream f(solutions_out, std::ios::binary);
    f.write(reinterpret_cast<const char*>(all.data()), std::streamsize(all.size() * sizeof(double)));
  }
  double max_delta = 0;
  for (double d : solver.refine_delta()) max_delta = std::max(max_delta, d);
  std::vector<double> errors(solver.errors().begin(), solver.errors().begin() + long(std::min(nrhs, solver.errors().size())));
  std::printf(
      "{\"converged\": %s, \"iterations\": %d, \"errors\": %s, \"residual_norms\": %s, \"xnorm\": %s, \"bnorm\": %s, "
      "\"refined_actions\": %d, \"first_refined_iteration\": %d, \"max_delta\": %.17g, \"actions\": %ld, \"nq\": %d}\n",
      converged ? "true" : "false", solver.statistics().iterations, list(errors).c_str(), list(rn).c_str(),
      list(xn).c_str(), list(bn).c_str(), solver.refined_actions(), solver.first_refined_iteration(), max_delta,
      solve_actions, int(solver.dimensions().nQ));
  return 0;
}

}  // namespace model

int main(int argc, char** argv) {
  if (argc != 9 && argc != 10) {
    std::fprintf(stderr, "usage: %s matrix n rhs nrhs threshold max_iter max_p mode [solutions]\n", argv[0]);
    return 2;
  }
  model::DenseProblem problem;
  problem.n = size_t(std::atol(argv[2]));
  problem.h.resize(problem.n * problem.n);
  std::ifstream f(argv[1], std::ios::binary);
  f.read(reinterpret_cast<char*>(problem.h.data()), std::streamsize(problem.h.size() * sizeof(double)));
  const size_t nrhs = size_t(std::atol(argv[4]));
  std::vector<model::Arr<double>> rhs;
  std::ifstream g(argv[3], std::ios::binary);
  for (size_t r = 0; r < nrhs; ++r) {
    rhs.emplace_back(problem.n);
    g.read(reinterpret_cast<char*>(rhs.back().v.data()), std::streamsize(problem.n * sizeof(double)));
  }
  if (!f || !g) {
    std::fprintf(stderr, "cannot read %s or %s\n", argv[1], argv[3]);
    return 2;
  }
  const double threshold = std::atof(argv[5]);
  const int max_iter = std::atoi(argv[6]), max_p = std::atoi(argv[7]);
  const std::string mode = argv[8];
  const char* out = argc == 10 ? argv[9] : nullptr;
  try {
    if (mode == "f64") return model::run<double>(problem, rhs, threshold, max_iter, max_p, mode, out);
    return model::run<float>(problem, rhs, threshold, max_iter, max_p, mode, out);
  } catch (const std::exception& e) {
    std::string msg = e.what();
    for (auto& c : msg)
      if (c == '"' || c == '\\') c = '\'';
    std::printf("{\"error\": \"%s\"}\n", msg.c_str());
    return 0;
  }
}
