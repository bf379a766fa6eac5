// The minimal double / float handler of tests/cpp/q32_refined_model.cpp (a copy: that file stays as it is), for
// tests/cpp/rc_refine_model.cpp: vectors whose logical element type is double over double or float storage,
// every operation in double, a result rounded once where the destination stores float; the
// quantise_for_storage overload of the refined mode; and the dense test problem.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
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
};

}  // namespace model
