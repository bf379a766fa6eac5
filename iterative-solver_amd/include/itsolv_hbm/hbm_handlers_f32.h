// Handlers for a Q space stored in f32 (hbm_vec_f32.h) beside f64 R vectors (hbm_vec.h), on the restated
// ArrayHandler base: ArrayHandlers<Vec, VecF32, SparseP> as make_handlers_q32() builds it.
//
//   rr, rp   the f64 handlers of hbm_handlers.h (with their fused hooks, which are typed on Vec)
//   rq       ArrayHandlerMx<Vec, VecF32>     overlaps of R with Q, gemm_outer of Q sources into R
//                                            (construct_solution, the block Gram-Schmidt update)
//   qr       ArrayHandlerMx<VecF32, Vec>     copy = the narrowing convert that makes a Q vector of an R
//   qq       ArrayHandlerMx<VecF32, VecF32>  construct_dspace, the Q space's own algebra
//   qp       ArrayHandlerMxSparse            VecF32 x P through a widened scratch Vec (not hot)
//   pp       ArrayHandlerSparse
// Every handler operation is one ssp_mx_* call (include/subspace_hip.h "mixed precision"): f32 operands are
// widened as they are loaded, the arithmetic is the f64 entry point's, an f32 destination is rounded
// once as it is stored.  A Vec operand's deferred scale rides along as the call's xs / ys.
//
// No existing header includes this one: solvers over Q = R = Vec do not see it.
#pragma once
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "hbm_handlers.h"
#include "hbm_vec_f32.h"

namespace molpro::linalg::hbm {

namespace mx {
inline constexpr ssp_dtype dtype(const Vec&) { return SSP_F64; }
inline constexpr ssp_dtype dtype(const VecF32&) { return SSP_F32; }
// read-only operand and the scale the kernel applies as it loads it
inline const void* rd(const Vec& v, double& s) {
  const void* p = v.data_deferred();
  s = v.scale();
  return p;
}
inline const void* rd(const VecF32& v, double& s) {
  s = 1.0;
  return v.data();
}
// read-modify-write destination (a Vec's pending scale is stored first)
inline void* rw(Vec& v) { return v.data_rw(); }
inline void* rw(VecF32& v) { return v.data(); }
// destination written in full
inline void* wo(Vec& v) { return v.data_wo(); }
inline void* wo(VecF32& v) { return v.data(); }
inline void scal(double a, Vec& v) { v.scale_by(a); }
inline void scal(double a, VecF32& v) {
  check_status<array::util::ArrayHandlerError>(ssp_scal_f32(v.ctx(), a, v.data(), v.local_size()), "ssp_scal_f32");
}
inline void fill(double a, Vec& v) { v.fill_deferred(a); }
inline void fill(double a, VecF32& v) {
  check_status<array::util::ArrayHandlerError>(ssp_fill_f32(v.ctx(), a, v.data(), v.local_size()), "ssp_fill_f32");
}
// a widened copy of an f32 vector (for the operations that are not hot: selection, sparse algebra)
inline Vec widened(const VecF32& v) {
  Vec w(v.device(), v.size());
  check_status<array::util::ArrayHandlerError>(
      ssp_mx_copy(v.ctx(), w.data_wo(), SSP_F64, v.data(), SSP_F32, 1.0, v.local_size()), "ssp_mx_copy");
  return w;
}
inline void narrow_into(VecF32& v, const Vec& w) {
  check_status<array::util::ArrayHandlerError>(
      ssp_mx_copy(v.ctx(), v.data(), SSP_F32, w.data(), SSP_F64, 1.0, v.local_size()), "ssp_mx_copy");
}
}  // namespace mx

// Dense handler over (AL, AR) in {Vec, VecF32}, at least one of them VecF32.
template <class AL, class AR>
class ArrayHandlerMx : public array::ArrayHandler<AL, AR> {
  using Base = array::ArrayHandler<AL, AR>;
  static_assert(std::is_same_v<AL, VecF32> || std::is_same_v<AR, VecF32>, "the f64 pair is ArrayHandlerHbm");
  static void check(int status, const char* what) { check_status<array::util::ArrayHandlerError>(status, what); }

 public:
  using typename Base::ProxyHandle;
  using Base::lazy_handle;
  ProxyHandle lazy_handle() override { return this->lazy_handle(*this); }

  AL copy(const AR& source) override {
    AL x(source.device(), source.size());
    copy(x, source);
    return x;
  }
  // x = (storage of x)(y): the convert (narrowing rounds to nearest-even); y's pending scale is applied
  void copy(AL& x, const AR& y) override {
    this->m_counter->copy++;
    same(x, y, "copy");
    double ys = 1.0;
    const void* yp = mx::rd(y, ys);
    check(ssp_mx_copy(y.ctx(), mx::wo(x), mx::dtype(x), yp, mx::dtype(y), ys, y.local_size()), "ssp_mx_copy");
  }
  void scal(double alpha, AL& x) override {
    this->m_counter->scal++;
    mx::scal(alpha, x);
  }
  void fill(double alpha, AL& x) override { mx::fill(alpha, x); }
  void axpy(double alpha, const AR& x, AL& y) override {
    this->m_counter->axpy++;
    if (x.size() < y.size()) this->error("ArrayHandlerMx::axpy() incompatible x and y arrays, x.size() < y.size()");
    same(y, x, "axpy");
    double xs = 1.0;
    const void* xp = mx::rd(x, xs);
    void* yp = mx::rw(y);
    if (xs == 1.0) {
      check(ssp_mx_axpy(y.ctx(), alpha, xp, mx::dtype(x), yp, mx::dtype(y), y.local_size()), "ssp_mx_axpy");
    } else {  // the one-source gemm_outer: fma(alpha, x * xs, y), ssp_axpy_scaled's arithmetic
      check(ssp_mx_gemm_outer(y.ctx(), &alpha, &xp, mx::dtype(x), &xs, 1, &yp, mx::dtype(y), 1, y.local_size(), 0),
            "ssp_mx_gemm_outer");
    }
  }
  double dot(const AL& x, const AR& y) override {
    this->m_counter->dot++;
    if (x.size() > y.size()) this->error("ArrayHandlerMx::dot() incompatible x and y arrays, x.size() > y.size()");
    same(x, y, "dot");
    double xs = 1.0, ys = 1.0, out = 0;
    const void* xp = mx::rd(x, xs);
    const void* yp = mx::rd(y, ys);
    if (xs == 1.0 && ys == 1.0)
      check(ssp_mx_dot(x.ctx(), xp, mx::dtype(x), yp, mx::dtype(y), x.local_size(), &out), "ssp_mx_dot");
    else
      check(ssp_mx_gemm_inner(x.ctx(), &xp, mx::dtype(x), &xs, 1, &yp, mx::dtype(y), &ys, 1, x.local_size(), &out),
            "ssp_mx_gemm_inner");
    return out;
  }
  void gemm_outer(const itsolv::subspace::Matrix<double> alphas, const itsolv::CVecRef<AR>& xx,
                  const itsolv::VecRef<AL>& yy) override {
    this->m_counter->gemm_outer++;
    if (yy.empty() || xx.empty()) return;
    if (alphas.rows() != xx.size())
      throw std::out_of_range("gemm_outer: dimensions of xx and alphas are different: " + std::to_string(alphas.rows()) +
                              " " + std::to_string(xx.size()));
    if (alphas.cols() > yy.size())
      throw std::out_of_range("gemm_outer: dimensions of yy and alphas are different: " + std::to_string(alphas.cols()) +
                              " " + std::to_string(yy.size()));
    const size_t m = alphas.cols();
    for (auto& x : xx) same(yy.front().get(), x.get(), "gemm_outer");
    std::vector<const void*> xp;
    std::vector<double> xs;
    for (auto& x : xx) {
      double s = 1.0;
      xp.push_back(mx::rd(x.get(), s));
      xs.push_back(s);
    }
    std::vector<void*> yp;
    for (size_t j = 0; j < m; ++j) yp.push_back(mx::rw(yy[j].get()));
    const auto& y0 = yy.front().get();
    check(ssp_mx_gemm_outer(y0.ctx(), alphas.data().data(), xp.data(), mx::dtype(xx.front().get()), xs.data(),
                            int(xx.size()), yp.data(), mx::dtype(y0), int(m), y0.local_size(), 0),
          "ssp_mx_gemm_outer");
  }
  itsolv::subspace::Matrix<double> gemm_inner(const itsolv::CVecRef<AL>& xx, const itsolv::CVecRef<AR>& yy) override {
    this->m_counter->gemm_inner++;
    std::vector<double> buf(xx.size() * yy.size(), 0.0);
    if (!xx.empty() && !yy.empty()) {
      for (auto& y : yy) same(xx.front().get(), y.get(), "gemm_inner");
      std::vector<const void*> xp, yp;
      std::vector<double> xs, ys;
      for (auto& x : xx) {
        double s = 1.0;
        xp.push_back(mx::rd(x.get(), s));
        xs.push_back(s);
      }
      for (auto& y : yy) {
        double s = 1.0;
        yp.push_back(mx::rd(y.get(), s));
        ys.push_back(s);
      }
      const auto& x0 = xx.front().get();
      check(ssp_mx_gemm_inner(x0.ctx(), xp.data(), mx::dtype(x0), xs.data(), int(xx.size()), yp.data(),
                              mx::dtype(yy.front().get()), ys.data(), int(yy.size()), x0.local_size(), buf.data()),
            "ssp_mx_gemm_inner");
    }
    return itsolv::subspace::Matrix<double>(std::move(buf), {xx.size(), yy.size()});
  }
  // Selection is not hot (the initial guess and the P space, once per solve): on widened copies.
  std::map<size_t, double> select_max_dot(size_t n, const AL& x, const AR& y) override {
    if (n > x.size() || n > y.size()) this->error("ArrayHandlerMx::select_max_dot() n is too large");
    same(x, y, "select_max_dot");
    return ArrayHandlerHbm().select_max_dot(n, f64(x), f64(y));
  }
  std::map<size_t, double> select(size_t n, const AL& x, bool max = false, bool ignore_sign = false) override {
    if (n > x.size()) this->error("ArrayHandlerMx::select() n is too large");
    return ArrayHandlerHbm().select(n, f64(x), max, ignore_sign);
  }

 protected:
  static const Vec& f64(const Vec& v) { return v; }
  static Vec f64(const VecF32& v) { return mx::widened(v); }
  template <class A, class B>
  void same(const A& a, const B& b, const char* op) {
    if (a.size() != b.size() || a.offset() != b.offset() || a.local_size() != b.local_size())
      this->error(std::string("ArrayHandlerMx::") + op + "() arrays have different distributions");
  }

  // Registered lazy dots: one gemm_inner over the distinct x and y (each vector read once).
  void fused_dot(const std::vector<std::tuple<size_t, size_t, size_t>>& reg,
                 const std::vector<std::reference_wrapper<const AL>>& xx,
                 const std::vector<std::reference_wrapper<const AR>>& yy,
                 std::vector<std::reference_wrapper<double>>& out) override {
    const auto m = gemm_inner(itsolv::CVecRef<AL>(xx.begin(), xx.end()), itsolv::CVecRef<AR>(yy.begin(), yy.end()));
    for (const auto& [x, y, z] : reg) out[z].get() = m(x, y);
  }
  // Registered lazy axpys as one gemm_outer, under ArrayHandlerHbm::fused_axpy's condition (each pair
  // once, every destination's sources in increasing order): bit for bit the axpy sequence into f64
  // destinations; an f32 destination is rounded once instead of once per axpy.
  void fused_axpy(const std::vector<std::tuple<size_t, size_t, size_t>>& reg, const std::vector<double>& alphas,
                  const std::vector<std::reference_wrapper<const AR>>& xx,
                  std::vector<std::reference_wrapper<AL>>& yy) override {
    const size_t nx = xx.size(), ny = yy.size();
    itsolv::subspace::Matrix<double> coef({nx, ny});
    std::vector<char> seen(nx * ny, 0);
    std::vector<long> last(ny, -1);
    bool batched = nx > 0 && ny > 0;
    for (const auto& [a, x, y] : reg) {
      if (seen[x * ny + y] || long(x) < last[y]) {
        batched = false;
        break;
      }
      seen[x * ny + y] = 1;
      last[y] = long(x);
      coef(x, y) = alphas[a];
    }
    if (!batched) {
      for (const auto& [a, x, y] : reg) axpy(alphas[a], xx[x].get(), yy[y].get());
      return;
    }
    for (size_t y = 1; y < ny; ++y) same(yy[y].get(), yy[0].get(), "fused_axpy");
    gemm_outer(coef, itsolv::CVecRef<AR>(xx.begin(), xx.end()), itsolv::VecRef<AL>(yy.begin(), yy.end()));
  }
};

// VecF32 x sparse P (Q x P).  Not hot: through a widened scratch Vec and the f64 sparse entry points,
// narrowed back where the f32 vector is the destination.
class ArrayHandlerMxSparse : public array::ArrayHandler<VecF32, SparseP> {
  using Base = array::ArrayHandler<VecF32, SparseP>;

 public:
  using typename Base::ProxyHandle;
  using Base::lazy_handle;
  ProxyHandle lazy_handle() override { return this->lazy_handle(*this); }

  VecF32 copy(const SparseP&) override {
    throw std::logic_error("ArrayHandlerMxSparse: cannot construct a distributed array from a sparse one");
  }
  void copy(VecF32& x, const SparseP& y) override {
    m_counter->copy++;
    Vec w(x.device(), x.size());
    m_f64.copy(w, y);
    mx::narrow_into(x, w);
  }
  void scal(double, VecF32&) override {}
  void fill(double, VecF32&) override {}
  void axpy(double alpha, const SparseP& x, VecF32& y) override {
    m_counter->axpy++;
    Vec w = mx::widened(y);
    m_f64.axpy(alpha, x, w);
    mx::narrow_into(y, w);
  }
  double dot(const VecF32& x, const SparseP& y) override {
    m_counter->dot++;
    return m_f64.dot(mx::widened(x), y);
  }
  void gemm_outer(const itsolv::subspace::Matrix<double> alphas, const itsolv::CVecRef<SparseP>& xx,
                  const itsolv::VecRef<VecF32>& yy) override {
    m_counter->gemm_outer++;
    if (xx.empty() || yy.empty()) return;
    if (alphas.rows() != xx.size() || alphas.cols() > yy.size())
      throw std::out_of_range("gemm_outer (sparse): dimensions of alphas do not match xx, yy");
    std::vector<Vec> w;
    for (size_t j = 0; j < alphas.cols(); ++j) w.push_back(mx::widened(yy[j].get()));
    m_f64.gemm_outer(alphas, xx, itsolv::VecRef<Vec>(w.begin(), w.end()));
    for (size_t j = 0; j < alphas.cols(); ++j) mx::narrow_into(yy[j].get(), w[j]);
  }
  itsolv::subspace::Matrix<double> gemm_inner(const itsolv::CVecRef<VecF32>& xx,
                                              const itsolv::CVecRef<SparseP>& yy) override {
    m_counter->gemm_inner++;
    // one row at a time through one reused scratch Vec: a sparse inner product is a per-row sum over the
    // P entries, so the rows are independent and only one widened vector is alive at any time.  The
    // price is one sparse inner product, with its host round trip, per row instead of one for all rows:
    // this handler is not on the hot path (Q x P overlaps of the few new Q vectors).
    itsolv::subspace::Matrix<double> out({xx.size(), yy.size()});
    if (xx.empty() || yy.empty()) return out;
    const VecF32& x0 = xx.front().get();
    Vec w(x0.device(), x0.size());
    for (size_t i = 0; i < xx.size(); ++i) {
      const VecF32& x = xx[i].get();
      if (!x.compatible(x0)) error("ArrayHandlerMxSparse::gemm_inner() arrays have different distributions");
      check_status<array::util::ArrayHandlerError>(
          ssp_mx_copy(x.ctx(), w.data_wo(), SSP_F64, x.data(), SSP_F32, 1.0, x.local_size()), "ssp_mx_copy");
      const auto row = m_f64.gemm_inner(itsolv::CVecRef<Vec>{std::cref(w)}, yy);
      for (size_t j = 0; j < yy.size(); ++j) out(i, j) = row(0, j);
    }
    return out;
  }
  std::map<size_t, double> select_max_dot(size_t n, const VecF32& x, const SparseP& y) override {
    return m_f64.select_max_dot(n, mx::widened(x), y);
  }
  std::map<size_t, double> select(size_t n, const VecF32& x, bool max = false, bool ignore_sign = false) override {
    return m_f64.select(n, mx::widened(x), max, ignore_sign);
  }

 private:
  ArrayHandlerHbmSparse m_f64;
};

// The bundle for R = hbm::Vec, Q = hbm::VecF32, P = std::map<size_t, double>.
inline std::shared_ptr<itsolv::ArrayHandlers<Vec, VecF32, SparseP>> make_handlers_q32() {
  return itsolv::ArrayHandlers<Vec, VecF32, SparseP>::create()
      .rr(std::make_shared<ArrayHandlerHbm>())
      .qq(std::make_shared<ArrayHandlerMx<VecF32, VecF32>>())
      .pp(std::make_shared<ArrayHandlerSparse>())
      .rq(std::make_shared<ArrayHandlerMx<Vec, VecF32>>())
      .rp(std::make_shared<ArrayHandlerHbmSparse>())
      .qr(std::make_shared<ArrayHandlerMx<VecF32, Vec>>())
      .qp(std::make_shared<ArrayHandlerMxSparse>())
      .build_shared();
}

// construct_solution over an f32 Q space (array::fused_construct_solution hook): one
// ssp_q32_construct_solution.  The Q and D sources -- every stream of the pass but the destinations --
// are read as f32 by a write-only pass (no zero fill, no read of the destinations), and the indices the
// sparse P vectors touch are recomputed P first: the reference sequence on the widened sources, bit for
// bit, as the f64 path's ssp_construct_solution_scaled.
inline bool fused_construct_solution(array::ArrayHandler<Vec, SparseP>&, const itsolv::subspace::Matrix<double>& cp,
                                     const itsolv::CVecRef<SparseP>& pp, const itsolv::subspace::Matrix<double>& cqd,
                                     const itsolv::CVecRef<VecF32>& qd, const itsolv::VecRef<Vec>& yy) {
  if (yy.empty() || cqd.cols() > yy.size() || cqd.rows() != qd.size() || cp.rows() != pp.size() ||
      (!pp.empty() && cp.cols() != cqd.cols()))
    return false;
  std::vector<size_t> ptr{0}, idx;
  std::vector<double> val;
  if (!pp.empty()) detail::pack(pp, ptr, idx, val);
  std::vector<const float*> xp;
  for (auto& q : qd) xp.push_back(q.get().data());
  auto yp = detail::wo_ptrs(itsolv::VecRef<Vec>(yy.begin(), yy.begin() + long(cqd.cols())));
  const auto& y0 = yy.front().get();
  check(ssp_q32_construct_solution(y0.ctx(), cp.data().data(), ptr.data(), idx.data(), val.data(), int(pp.size()),
                                   cqd.data().data(), xp.data(), int(qd.size()), yp.data(), int(cqd.cols()),
                                   y0.local_size(), y0.offset()),
        "ssp_q32_construct_solution");
  return true;
}

// The block Gram-Schmidt update over an f32 Q space (array::fused_block_update hook, rspace.h
// block_gram_schmidt): one ssp_q32_block_update -- bit-identical to gemm_outer(P) then gemm_outer(Q, D)
// on widened sources, and the destinations' deferred normalisation scale is applied as they are read
// instead of costing a pass of its own.
inline bool fused_block_update(array::ArrayHandler<Vec, SparseP>&, const itsolv::subspace::Matrix<double>& cp,
                               const itsolv::CVecRef<SparseP>& pp, const itsolv::subspace::Matrix<double>& cqd,
                               const itsolv::CVecRef<VecF32>& qd, const itsolv::VecRef<Vec>& yy) {
  const size_t m = yy.size();
  if (m == 0 || cqd.rows() != qd.size() || cp.rows() != pp.size() || (!qd.empty() && cqd.cols() != m) ||
      (!pp.empty() && cp.cols() != m))
    return false;
  std::vector<size_t> ptr{0}, idx;
  std::vector<double> val;
  if (!pp.empty()) detail::pack(pp, ptr, idx, val);
  std::vector<const float*> xp;
  for (auto& q : qd) xp.push_back(q.get().data());
  std::vector<double> ys;
  auto yp = detail::rw_deferred_ptrs(yy, ys);
  const auto& y0 = yy.front().get();
  check(ssp_q32_block_update(y0.ctx(), cp.data().data(), ptr.data(), idx.data(), val.data(), int(pp.size()),
                             cqd.data().data(), xp.data(), int(qd.size()), yp.data(), ys.data(), int(m),
                             y0.local_size(), y0.offset()),
        "ssp_q32_block_update");
  detail::scales_applied(yy);
  return true;
}

// The new rows of the subspace matrices over f64 and f32 columns as one ssp_q32_gemm_inner_cols
// (array::fused_overlap_rows_mixed hook; subspace.h new_qspace_data, rspace.h append_overlap_with_r): the
// rows are read once per launch of 64 columns whatever the columns' storage, where the block-by-block
// overlaps are one call, one host round trip and one read of the rows per block.  From fused_min_size(),
// as the other fused solver passes.
inline bool fused_overlap_rows_mixed(array::ArrayHandler<Vec, VecF32>&, const itsolv::CVecRef<Vec>& rows,
                                     const std::vector<itsolv::CVecRef<Vec>>& rcols,
                                     const std::vector<itsolv::CVecRef<VecF32>>& qcols,
                                     itsolv::subspace::Matrix<double>& out) {
  if (rows.empty() || rows.front().get().size() < fused_min_size()) return false;
  const Vec& x0 = rows.front().get();
  auto same = [&](size_t size, size_t offset, size_t local) {
    if (size != x0.size() || offset != x0.offset() || local != x0.local_size())
      throw array::util::ArrayHandlerError{"fused_overlap_rows_mixed: arrays have different distributions"};
  };
  std::vector<double> xs, ys;
  auto xp = detail::deferred_ptrs(rows, xs);
  std::vector<const void*> yp;
  std::vector<ssp_dtype> ty;
  for (const auto& c : rcols)
    for (auto& v : c) {
      same(v.get().size(), v.get().offset(), v.get().local_size());
      yp.push_back(v.get().data_deferred());
      ys.push_back(v.get().scale());
      ty.push_back(SSP_F64);
    }
  for (const auto& c : qcols)
    for (auto& v : c) {
      same(v.get().size(), v.get().offset(), v.get().local_size());
      yp.push_back(v.get().data());
      ys.push_back(1.0);
      ty.push_back(SSP_F32);
    }
  if (yp.empty()) return false;
  for (auto& r : rows) same(r.get().size(), r.get().offset(), r.get().local_size());
  std::vector<double> buf(rows.size() * yp.size(), 0.0);
  check(ssp_q32_gemm_inner_cols(x0.ctx(), xp.data(), xs.data(), int(rows.size()), yp.data(), ty.data(), ys.data(),
                                int(yp.size()), x0.local_size(), buf.data()),
        "ssp_q32_gemm_inner_cols");
  out = itsolv::subspace::Matrix<double>(std::move(buf), {rows.size(), yp.size()});
  return true;
}

// The residuals of linear equations and their norms as one ssp_mx_rhs_residual_norms
// (array::fused_rhs_residual_norms hook, LinearEquationsDavidson::construct_residual): r_i = s_i (r_i - b_i)
// element for element the handler's axpy(-1) and scal, the norms update_errors' dots up to summation order, a
// residual's pending scale applied as it is loaded.  The right-hand sides are the stored ones (VecF32) or, in the
// refined mode, their f64 twins (Vec); both come through the R x Q handler of the q32 set, so a solver over
// make_handlers() never gets here.  From fused_min_size(), as the other fused solver passes.
namespace detail {
template <class B>
bool rhs_residual_norms(const std::vector<double>& s, const itsolv::CVecRef<B>& bb, ssp_dtype tb,
                        const itsolv::VecRef<Vec>& yy, std::vector<double>& norms2) {
  const size_t m = yy.size();
  if (m == 0 || bb.size() < m || s.size() < m || yy.front().get().size() < fused_min_size()) return false;
  const Vec& y0 = yy.front().get();
  std::vector<const void*> bp;
  for (size_t i = 0; i < m; ++i) {
    const B& b = bb[i].get();
    if (b.size() != y0.size() || b.offset() != y0.offset() || b.local_size() != y0.local_size())
      throw array::util::ArrayHandlerError{"fused_rhs_residual_norms: arrays have different distributions"};
    if constexpr (std::is_same_v<B, Vec>) {
      if (b.scale() != 1.0) return false;  // (a right-hand side is a copy: it carries no pending scale)
      bp.push_back(b.data_deferred());
    } else {
      bp.push_back(b.data());
    }
  }
  std::vector<double> ys;
  auto yp = rw_deferred_ptrs(yy, ys);
  norms2.assign(m, 0.0);
  check(ssp_mx_rhs_residual_norms(y0.ctx(), bp.data(), tb, s.data(), yp.data(), ys.data(), int(m), y0.local_size(),
                                  norms2.data()),
        "ssp_mx_rhs_residual_norms");
  scales_applied(yy);
  return true;
}
}  // namespace detail
inline bool fused_rhs_residual_norms(array::ArrayHandler<Vec, VecF32>&, const std::vector<double>& s,
                                     const itsolv::CVecRef<VecF32>& bb, const itsolv::VecRef<Vec>& yy,
                                     std::vector<double>& norms2) {
  return detail::rhs_residual_norms(s, bb, SSP_F32, yy, norms2);
}
inline bool fused_rhs_residual_norms(array::ArrayHandler<Vec, VecF32>&, const std::vector<double>& s,
                                     const itsolv::CVecRef<Vec>& bb, const itsolv::VecRef<Vec>& yy,
                                     std::vector<double>& norms2) {
  return detail::rhs_residual_norms(s, bb, SSP_F64, yy, norms2);
}

// R vectors rounded in place to the values their narrowing copy into the Q space stores
// (array::quantise_for_storage hook, the refined mode of solvers.h): one ssp_quantise_f32 for all of them, a
// pending normalisation scale applied as the vector is loaded.  What qr().copy() makes of the result is exact.
inline bool quantise_for_storage(array::ArrayHandler<VecF32, Vec>&, const itsolv::VecRef<Vec>& xx) {
  if (xx.empty()) return true;
  const Vec& x0 = xx.front().get();
  for (auto& x : xx)
    if (!x.get().compatible(x0))
      throw array::util::ArrayHandlerError{"quantise_for_storage: arrays have different distributions"};
  std::vector<double> xs;
  auto xp = detail::rw_deferred_ptrs(xx, xs);
  check(ssp_quantise_f32(x0.ctx(), xp.data(), xs.data(), int(xx.size()), x0.local_size()), "ssp_quantise_f32");
  detail::scales_applied(xx);
  return true;
}

// New Q vectors as linear combinations of existing ones (array::fused_new_combinations hook,
// construct_dspace): allocated without a copy and written by one write-only f32 -> f32 gemm_outer, each
// element the f64 sum of its sources in order, rounded once.
inline bool fused_new_combinations(array::ArrayHandler<VecF32, VecF32>&, const itsolv::subspace::Matrix<double>& coeff,
                                   const std::vector<const VecF32*>& src, std::vector<VecF32>& out) {
  const size_t nout = coeff.rows(), k = src.size();
  if (k == 0 || coeff.cols() != k) return false;
  std::vector<const void*> xp;
  for (auto* v : src) xp.push_back(v->data());
  std::vector<double> alphas(k * nout);  // alphas[i * m + j]: source i, destination j
  for (size_t j = 0; j < nout; ++j)
    for (size_t i = 0; i < k; ++i) alphas[i * nout + j] = coeff(j, i);
  const size_t first = out.size();
  for (size_t j = 0; j < nout; ++j) out.push_back(src.front()->alloc_like());
  std::vector<void*> yp;
  for (size_t j = first; j < out.size(); ++j) yp.push_back(out[j].data());
  const VecF32& v0 = *src.front();
  check(ssp_mx_gemm_outer(v0.ctx(), alphas.data(), xp.data(), SSP_F32, nullptr, int(k), yp.data(), SSP_F32, int(nout),
                          v0.local_size(), 1),
        "ssp_mx_gemm_outer");
  return true;
}

// The same with the new vectors' f64 twins (array::fused_new_combinations_widened hook, the consistent D space
// of rspace.h construct_dspace_refined): one ssp_q32_combine_widen writes each new f32 vector and, into twin[j],
// the value it stored, widened -- the pass reads the sources once and neither destination set.  From
// fused_min_size(), as the other fused solver passes (below it: fused_new_combinations, then the widening copies).
inline bool fused_new_combinations_widened(array::ArrayHandler<VecF32, VecF32>&,
                                           const itsolv::subspace::Matrix<double>& coeff,
                                           const std::vector<const VecF32*>& src, std::vector<VecF32>& out,
                                           const itsolv::VecRef<Vec>& twin) {
  const size_t nout = coeff.rows(), k = src.size();
  if (k == 0 || coeff.cols() != k || twin.size() < nout || src.front()->size() < fused_min_size()) return false;
  const VecF32& v0 = *src.front();
  std::vector<const float*> xp;
  for (auto* v : src) xp.push_back(v->data());
  std::vector<double> alphas(k * nout);  // alphas[i * m + j]: source i, destination j
  for (size_t j = 0; j < nout; ++j)
    for (size_t i = 0; i < k; ++i) alphas[i * nout + j] = coeff(j, i);
  for (size_t j = 0; j < nout; ++j) {
    const Vec& w = twin[j].get();
    if (w.size() != v0.size() || w.offset() != v0.offset() || w.local_size() != v0.local_size())
      throw array::util::ArrayHandlerError{"fused_new_combinations_widened: arrays have different distributions"};
  }
  const size_t first = out.size();
  for (size_t j = 0; j < nout; ++j) out.push_back(v0.alloc_like());
  std::vector<float*> yp;
  std::vector<double*> wp;
  for (size_t j = 0; j < nout; ++j) {
    yp.push_back(out[first + j].data());
    wp.push_back(twin[j].get().data_wo());
  }
  check(ssp_q32_combine_widen(v0.ctx(), alphas.data(), xp.data(), int(k), yp.data(), wp.data(), int(nout),
                              v0.local_size()),
        "ssp_q32_combine_widen");
  return true;
}

// A DIIS history stored as f32 differences behind f64 anchors (diis_differences.h).
// array::fused_store_differences hook: one ssp_q32_store_differences writes the new differences (allocated here,
// never copied or zeroed) and refreshes the anchors -- 28 bytes per element and vector, bit for bit what the
// copy, axpy(-1), narrowing copy and copy of the fallback store.  From fused_min_size(), as the other fused passes.
inline bool fused_store_differences(array::ArrayHandler<VecF32, Vec>&, const itsolv::CVecRef<Vec>& vv,
                                    const itsolv::VecRef<Vec>& aa, std::vector<VecF32>& out) {
  const size_t m = vv.size();
  if (m == 0 || aa.size() != m || vv.front().get().size() < fused_min_size()) return false;
  const Vec& v0 = vv.front().get();
  for (size_t j = 0; j < m; ++j)
    if (!vv[j].get().compatible(v0) || !aa[j].get().compatible(v0))
      throw array::util::ArrayHandlerError{"fused_store_differences: arrays have different distributions"};
  std::vector<const double*> vp;
  std::vector<double*> ap;
  std::vector<float*> dp;
  for (auto& v : vv) vp.push_back(v.get().data());  // (a pending scale is stored first)
  for (auto& a : aa) ap.push_back(a.get().data_rw());  // (an anchor that still shares a caller's block gets its own)
  const size_t first = out.size();
  for (size_t j = 0; j < m; ++j) out.emplace_back(v0.device(), v0.size());
  for (size_t j = 0; j < m; ++j) dp.push_back(out[first + j].data());
  check(ssp_q32_store_differences(v0.ctx(), vp.data(), ap.data(), dp.data(), int(m), v0.local_size()),
        "ssp_q32_store_differences");
  return true;
}

// array::fused_anchor_combine hook: one ssp_q32_anchor_combine for the panels of a step (the parameters and the
// residuals), write-only destinations -- bit for bit the anchor's copy and the gemm_outer of the fallback.  From
// fused_min_size(), as the other fused passes.
inline bool fused_anchor_combine(array::ArrayHandler<Vec, VecF32>&, const std::vector<double>& gammas,
                                 const itsolv::CVecRef<Vec>& aa, const std::vector<itsolv::CVecRef<VecF32>>& dd,
                                 const itsolv::VecRef<Vec>& yy) {
  const size_t m = yy.size(), k = gammas.size();
  if (m == 0 || aa.size() != m || dd.size() != m || yy.front().get().size() < fused_min_size()) return false;
  const Vec& y0 = yy.front().get();
  std::vector<const double*> ap;
  std::vector<const float*> dp;
  for (size_t j = 0; j < m; ++j) {
    if (dd[j].size() != k || !aa[j].get().compatible(y0) || !yy[j].get().compatible(y0))
      throw array::util::ArrayHandlerError{"fused_anchor_combine: arrays have different distributions"};
    ap.push_back(aa[j].get().data());
    for (auto& d : dd[j]) {
      if (!d.get().compatible(y0))
        throw array::util::ArrayHandlerError{"fused_anchor_combine: arrays have different distributions"};
      dp.push_back(d.get().data());
    }
  }
  // write-only destinations: one that still shares an anchor's block is given a fresh block, nothing is copied
  auto yp = detail::wo_ptrs(yy);
  check(ssp_q32_anchor_combine(y0.ctx(), gammas.data(), ap.data(), dp.data(), int(k), yp.data(), int(m), y0.local_size()),
        "ssp_q32_anchor_combine");
  return true;
}

}  // namespace molpro::linalg::hbm
