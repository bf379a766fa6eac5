// The refined mode under a Q-space limit (itsolv_hbm/solvers.h set_refine_dspace) on the CPU:
// LinearEigensystemDavidson<R, Q, P> with R over double storage and Q over float storage, on the minimal handler
// of tests/cpp/q32_refined_model.cpp (repeated here: each is a program of its own), with this file's own
// quantise_for_storage and fused_new_combinations_widened overloads.  No device: what runs is the solver's
// consistent D space -- the coefficients, the one pass over the source parameters, the true actions, the D
// blocks of S and H (call by call), the refined rows with nD != 0 and the bound with its D terms.
//
//   q32_refined_dspace_model <matrix file: n*n doubles, row-major> <n> <nroots> <threshold> <max_iter> <limit> <mode>
//                            [max_p: solve()'s P space of that many unit vectors; default none]
// mode: f64 (Q stored as double, max_size_qspace = limit), dspace (Q as float, set_refine + set_refine_dspace,
// the same limit), dspace0 (the same with set_refine_dspace_slack(0): the plain solver's rebuild schedule),
// refused (Q as float, set_refine and the limit without the opt-in: the error goes to stderr).
// Prints one JSON line: converged, iterations, eigenvalues, errors, residual_norms (recomputed here from the
// matrix), refined_actions, dspace_rebuilds, dspace_actions, max_delta, actions (all calls' vectors).
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

// The hook of the consistent D space for this file's vectors: each new vector the double sum of its sources in
// order, rounded once, and its twin the stored value widened.
inline bool fused_new_combinations_widened(ArrayHandler<Arr<float>, Arr<float>>&, const Matrix<double>& c,
                                           const std::vector<const Arr<float>*>& src, std::vector<Arr<float>>& out,
                                           const VecRef<Arr<double>>& twin) {
  const size_t n = src.front()->size();
  for (size_t i = 0; i < c.rows(); ++i) {
    Arr<float> y(n);
    Arr<double>& w = twin.at(i).get();
    w.v.resize(n);
    for (size_t e = 0; e < n; ++e) {
      double t = 0;
      for (size_t j = 0; j < src.size(); ++j) t = std::fma(c(i, j), double(src[j]->v[e]), t);
      y.v[e] = float(t);
      w.v[e] = double(y.v[e]);
    }
    out.push_back(std::move(y));
  }
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
  // the P space of solve() (max_p): unit vectors
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

template <class SQ>
int run(const DenseProblem& problem, int nroots, double threshold, int max_iter, int limit, bool refine, bool dspace,
        int slack = -1, int max_p = 0) {
  using R = Arr<double>;
  using Q = Arr<SQ>;
  molpro::linalg::itsolv::LinearEigensystemDavidson<R, Q, SP> solver(handlers<SQ>());
  solver.set_n_roots(size_t(nroots));
  solver.set_convergence_threshold(threshold);
  solver.set_max_iter(max_iter);
  solver.set_hermiticity(true);
  solver.set_verbosity(molpro::linalg::itsolv::Verbosity::None);
  if (refine) solver.set_refine(true);
  if (dspace) solver.set_refine_dspace(true);
  solver.set_refine_dspace_slack(slack);
  solver.set_max_size_qspace(limit);
  if (max_p > 0) solver.set_max_p(max_p);
  std::vector<R> x, a;
  for (int i = 0; i < nroots; ++i) {
    x.emplace_back(problem.n);
    a.emplace_back(problem.n);
  }
  const bool converged = solver.solve(x, a, problem, true);
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
      "\"refined_actions\": %d, \"dspace_rebuilds\": %d, \"dspace_actions\": %d, "
      "\"max_delta\": %.17g, \"actions\": %ld}\n",
      converged ? "true" : "false", solver.statistics().iterations, list(ev, size_t(nroots)).c_str(),
      list(solver.errors(), size_t(nroots)).c_str(), list(rn, size_t(nroots)).c_str(), solver.refined_actions(),
      solver.dspace_rebuilds(), solver.dspace_actions(), max_delta, solve_actions);
  return 0;
}

}  // namespace model

int main(int argc, char** argv) {
  if (argc != 8 && argc != 9) {
    std::fprintf(stderr, "usage: %s matrix n nroots threshold max_iter limit f64|dspace|dspace0|refused [max_p]\n", argv[0]);
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
  const int nroots = std::atoi(argv[3]), max_iter = std::atoi(argv[5]), limit = std::atoi(argv[6]);
  const double threshold = std::atof(argv[4]);
  const std::string mode = argv[7];
  const int max_p = argc == 9 ? std::atoi(argv[8]) : 0;
  try {
    if (mode == "f64") return model::run<double>(problem, nroots, threshold, max_iter, limit, false, false, -1, max_p);
    if (mode == "dspace") return model::run<float>(problem, nroots, threshold, max_iter, limit, true, true, -1, max_p);
    if (mode == "dspace0") return model::run<float>(problem, nroots, threshold, max_iter, limit, true, true, 0, max_p);
    if (mode == "refused") return model::run<float>(problem, nroots, threshold, max_iter, limit, true, false);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
