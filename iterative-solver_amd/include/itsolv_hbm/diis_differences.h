// NonLinearEquationsDIISDifferences: DIIS whose history is stored as successive differences, so that the history
// may be held in a narrower format than the iterates (Q over f32 beside R over f64) and still reach R's thresholds.
//
// Why not NonLinearEquationsDIIS<R, narrow Q>: near convergence every stored iterate is approximately x*, so
// rounding each to f32 puts an error of 2^-24 |x*| into the extrapolated parameters and the next residual cannot
// fall below about 2^-24 |J| |x*|.  The differences between successive iterates shrink with the error, and so
// does what their rounding loses.
//
// The representation.  Points are indexed newest first, as in NonLinearEquationsDIIS.
//   - two anchors in R's format: copies of the newest point (x_0, r_0);
//   - k - 1 pairs of differences in Q's format: dx_i = (Q)(x_i - x_{i+1}) and dr_i likewise, each rounded once,
//     when it is stored.  So x_j = x_0 - sum_{i<j} dx_i.
//   - The subspace matrix H = <r_i, r_j> stays in the point basis (SubspaceSolverDIIS, dense::solve_DIIS,
//     least_important_vector and svd_thresh are the base class's): old entries are kept, and the new row is
//     H_00 = <r_0, r_0>, H_0j = H_00 - sum_{i<j} <r_0, dr_i>: one inner product of the row r_0 against itself and
//     the k - 1 stored differences.
//   - Point-basis coefficients c (sum c = 1) become gamma_i = sum_{j>i} c_j on the host; then
//     x = x_0 - sum_i gamma_i dx_i and r = r_0 - sum_i gamma_i dr_i.  When converged, c = e_0: the anchor itself.
//   - Deleting point j >= 1: the oldest point drops the last pair; any other merges dx_{j-1} <- (Q)(dx_{j-1} + dx_j)
//     (an error relative to the differences).  Point 0 is never deleted from a history of two or more points (an
//     error); a history limit of one point empties the history, as it empties the base class's.
//
// Every vector operation goes through the ArrayHandlers; the two passes of the representation are the hooks
// array::fused_store_differences and array::fused_anchor_combine, with the call-by-call sequence where a handler
// has none (or declines: short vectors).  A P space is refused by name.  The options, add_vector / end_iteration /
// solution / solve, errors(), the statistics and max_size_qspace / svd_thresh are NonLinearEquationsDIIS's.
#pragma once
#include <memory>
#include <stdexcept>
#include <vector>

#include "solvers.h"

namespace molpro::linalg::itsolv {

template <class R, class Q = R, class P = std::map<size_t, typename R::value_type>>
class NonLinearEquationsDIISDifferences : public NonLinearEquationsDIIS<R, Q, P> {
  using Base = NonLinearEquationsDIIS<R, Q, P>;
  using Template = IterativeSolverTemplate<R, Q, P>;

 public:
  using typename Base::value_type;
  using typename Template::fapply_on_p_type;
  explicit NonLinearEquationsDIISDifferences(std::shared_ptr<ArrayHandlers<R, Q, P>> handlers,
                                             std::shared_ptr<Logger> logger = std::make_shared<Logger>())
      : Base(std::move(handlers), std::move(logger)) {}

  //! The new point (parameters, residual): pruned history, the new pair of differences, the new row of H, then
  //! the subspace solution and the extrapolated pair in parameters / residual (NonLinearEquationsDIIS::add_vector).
  int add_vector(R& parameters, R& residual, value_type value = 0) override {
    if (this->m_max_p != 0) refuse_p("max_p");
    auto& h = *this->m_handlers;
    auto& H = this->m_xspace->data[EqnData::H];
    for (auto del = this->least_important_vector(H);
         size() >= size_t(this->m_max_size_qspace) || del.second < this->m_svd_thresh;
         del = this->least_important_vector(H))
      erase_point(del.first);
    this->m_stats->r_creations += 1;
    store(parameters, residual);
    this->m_stats->q_creations += 2;
    // the new row of H, point basis: <r_0, r_0> and <r_0, dr_i> in one pass where the handlers batch rows
    const size_t k = size();
    CVecRef<Q> dr;
    for (const auto& d : m_diff) dr.emplace_back(d.action);
    const auto row = cwrap_arg(residual);
    std::vector<double> dots(k, 0.0);  // [<r_0, r_0>, <r_0, dr_0>, ...]
    Matrix<double> g;
    bool fused = false;
    {
      using array::fused_overlap_rows;
      using array::fused_overlap_rows_mixed;
      if constexpr (std::is_same_v<R, Q>) fused = fused_overlap_rows(h.rr(), row, std::vector<CVecRef<R>>{row, dr}, g);
      else fused = fused_overlap_rows_mixed(h.rq(), row, std::vector<CVecRef<R>>{row}, std::vector<CVecRef<Q>>{dr}, g);
    }
    if (fused) {
      for (size_t i = 0; i < k; ++i) dots[i] = g(0, i);
    } else {
      dots[0] = h.rr().dot(residual, residual);
      if (k > 1) {
        const auto q = subspace::util::overlap(row, dr, h.rq());
        for (size_t i = 1; i < k; ++i) dots[i] = q(0, i - 1);
      }
    }
    const double error = std::sqrt(std::abs(dots[0]));
    this->m_converged = error < this->m_convergence_threshold;
    Matrix<double> Hn({k, k});
    for (size_t i = 1; i < k; ++i)
      for (size_t j = 1; j < k; ++j) Hn(i, j) = H(i - 1, j - 1);
    double h0j = dots[0];
    Hn(0, 0) = h0j;
    for (size_t j = 1; j < k; ++j) {
      h0j -= dots[j];
      Hn(0, j) = Hn(j, 0) = h0j;
    }
    H = std::move(Hn);
    m_dims = subspace::Dimensions(0, k, 0);
    const auto nwork = this->solve_and_generate_working_set(wrap_arg(parameters), wrap_arg(residual));
    read_handler_counts(*this->m_stats, *this->m_handlers);
    this->m_end_iteration_needed = true;
    this->m_errors.front() = error;
    return int(nwork);
  }
  int add_vector(const VecRef<R>& parameters, const VecRef<R>& actions) override {
    if (parameters.empty() || actions.empty()) throw std::runtime_error("NonLinearEquationsDIISDifferences: no vector given");
    return add_vector(parameters.front().get(), actions.front().get());
  }
  using Template::add_vector;

  size_t add_p(const CVecRef<P>&, const std::vector<double>&, const VecRef<R>&, const VecRef<R>&, fapply_on_p_type) override {
    refuse_p("add_p");
    return 0;
  }

  //! parameters[0] = x_0 - sum gamma_i dx_i and residual[0] = r_0 - sum gamma_i dr_i, both in one pass where the
  //! handlers have it
  void solution(const std::vector<int>& roots, const VecRef<R>& parameters, const VecRef<R>& residual) override {
    this->check_roots(roots, parameters.size());
    if (roots.empty()) return;
    if (residual.empty()) throw std::runtime_error("asking for more roots than residuals");
    combine({std::ref(parameters.front().get()), std::ref(residual.front().get())}, true);
    read_handler_counts(*this->m_stats, *this->m_handlers);
  }
  using Template::solution;
  //! parameters[0] alone, rebuilt from the anchor and the stored differences (end_iteration goes through here:
  //! never from the caller's array)
  void solution_params(const std::vector<int>& roots, const VecRef<R>& parameters) override {
    this->check_roots(roots, parameters.size());
    if (roots.empty()) return;
    combine({std::ref(parameters.front().get())}, false);
  }

  const subspace::Dimensions& dimensions() const override { return m_dims; }

  //! Deletes point j, H's row and column with it (what add_vector's pruning calls; the subspace solution is the
  //! next add_vector's)
  void erase_point(size_t j) {
    auto& h = *this->m_handlers;
    const size_t k = size();
    if (j >= k) throw std::logic_error("NonLinearEquationsDIISDifferences: no such point");
    if (k == 1) {  // a history limit of one point: the history is emptied, as the base class empties its own
      m_anchor_x.reset();
      m_anchor_r.reset();
    } else if (j == 0) {  // (least_important_vector never names point 0 of two or more)
      throw std::logic_error("NonLinearEquationsDIISDifferences: point 0, the anchor, is never deleted");
    } else if (j == k - 1) {  // the oldest point: its pair goes
      m_diff.pop_back();
    } else {  // a middle point: its two pairs merge
      h.qq().axpy(1, m_diff[j].param, m_diff[j - 1].param);
      h.qq().axpy(1, m_diff[j].action, m_diff[j - 1].action);
      m_diff.erase(m_diff.begin() + long(j));
      ++m_merged;
    }
    this->m_xspace->data[EqnData::H].remove_row_col(j, j);
    m_dims = subspace::Dimensions(0, size(), 0);
  }

  //! points held (the anchor's included)
  size_t size() const { return m_anchor_x ? m_diff.size() + 1 : 0; }
  //! what the history holds: pairs of differences in Q's format (size() - 1) and anchors in R's format (2 or 0)
  size_t difference_pairs() const { return m_diff.size(); }
  size_t anchors() const { return m_anchor_x ? 2 : 0; }
  //! points deleted so far whose two pairs were merged (neither the newest nor the oldest)
  size_t merged_deletions() const { return m_merged; }

 private:
  struct Pair {
    Q param, action;
  };

  [[noreturn]] static void refuse_p(const char* what) {
    throw std::runtime_error(std::string("NonLinearEquationsDIISDifferences: a P space is not supported (") + what + ")");
  }

  // The new point: differences against the anchors (newest first), then the anchors become the point.
  void store(const R& x, const R& r) {
    auto& h = *this->m_handlers;
    if (!m_anchor_x) {
      m_anchor_x = std::make_unique<R>(h.rr().copy(x));
      m_anchor_r = std::make_unique<R>(h.rr().copy(r));
      return;
    }
    std::vector<Q> d;
    bool fused = false;
    {
      using array::fused_store_differences;
      fused = fused_store_differences(h.qr(), CVecRef<R>{std::cref(x), std::cref(r)},
                                      VecRef<R>{std::ref(*m_anchor_x), std::ref(*m_anchor_r)}, d);
    }
    if (!fused) {
      const R* point[2] = {&x, &r};
      R* anchor[2] = {m_anchor_x.get(), m_anchor_r.get()};
      for (int s = 0; s < 2; ++s) {
        R t{h.rr().copy(*point[s])};
        h.rr().axpy(-1, *anchor[s], t);
        d.emplace_back(h.qr().copy(t));
        h.rr().copy(*anchor[s], *point[s]);
      }
    }
    m_diff.insert(m_diff.begin(), Pair{std::move(d[0]), std::move(d[1])});
  }

  // yy = the anchors minus the gamma-weighted differences: yy[0] the parameters, yy[1] (with_residual) the residuals.
  void combine(const VecRef<R>& yy, bool with_residual) {
    auto& h = *this->m_handlers;
    const auto& c = this->m_subspace_solver->solutions();
    const size_t k = size();
    if (c.cols() != k || k == 0) throw std::logic_error("NonLinearEquationsDIISDifferences: no subspace solution");
    std::vector<double> gamma(k - 1, 0.0);
    for (size_t i = k - 1; i-- > 0;) gamma[i] = (i + 1 < k - 1 ? gamma[i + 1] : 0.0) + c(0, i + 1);
    CVecRef<R> aa{std::cref(*m_anchor_x)};
    std::vector<CVecRef<Q>> dd(1);
    for (const auto& d : m_diff) dd[0].emplace_back(d.param);
    if (with_residual) {
      aa.emplace_back(*m_anchor_r);
      dd.emplace_back();
      for (const auto& d : m_diff) dd[1].emplace_back(d.action);
    }
    bool fused = false;
    {
      using array::fused_anchor_combine;
      fused = fused_anchor_combine(h.rq(), gamma, aa, dd, yy);
    }
    if (fused) return;
    Matrix<double> al({k - 1, 1});
    for (size_t i = 0; i + 1 < k; ++i) al(i, 0) = -gamma[i];
    for (size_t s = 0; s < yy.size(); ++s) {
      h.rr().copy(yy[s].get(), aa[s].get());
      if (k > 1) h.rq().gemm_outer(al, dd[s], VecRef<R>{yy[s]});
    }
  }

  std::unique_ptr<R> m_anchor_x, m_anchor_r;
  std::vector<Pair> m_diff;  // m_diff[i]: (dx_i, dr_i), newest first
  subspace::Dimensions m_dims;
  size_t m_merged = 0;
};

}  // namespace molpro::linalg::itsolv
