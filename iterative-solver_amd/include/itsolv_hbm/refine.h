// The refined mode of the Davidson solvers, for a Q space stored in a narrower format than R (extension; off by
// default, and then every path is as it was).  Everything the mode keeps per solver is here; DavidsonSolver
// (solvers.h) owns one Refinement and calls it from the three places where the mode changes a solve:
//  1. each new R parameter vector is rounded to the Q storage format (array::quantise_for_storage) before
//     problem.action sees it, so its copy into the Q space is exact and a_j = H q_j to the precision of R;
//  2. the new rows of H come from the stored Q parameters and the new actions in R's precision
//     (subspace.h XSpace::set_refined), so S and H are the exact projection onto span{q_j};
//  3. only the stored actions then carry error: for root i, |r_est - r_true| <= delta_i (Refinement::bound) with
//     |a_j| kept on the host.  A root whose estimate the bound no longer vouches for (Refinement::triggers) gets
//     its residual from the action of its solution instead: one more action per such root and iteration, all
//     refined roots of a batch in one call -- converged roots included, since the solver recomputes every root's
//     residual in every iteration.  That is the price of actions stored in 4 bytes.
// Scope: the hermitian LinearEigensystemDavidson, no max_size_qspace, reset_D or reset_D_max_Q_size, an empty D
// space (each is an error naming the option); and the hermitian LinearEquationsDavidson in the same scope, without
// the augmented Hessian and without the consistent D space (DavidsonSolver::check_refine).  The refined residuals
// need the problem's action: solve() provides it; a caller driving add_vector by hand gives it with
// set_refine_action, and rounds the parameter vectors itself before it applies the action (step 1).  Without
// either, a needed refinement throws.
//
// The mode under a Q-space limit (options.dspace; opt-in).  With it the scope admits a finite max_size_qspace, and
// whenever the limit deletes Q vectors the D space is rebuilt consistently: the new D parameters are written by
// one pass over the deleted Q and old D PARAMETERS, rounded once, with their values in R's format beside them
// (rspace.h construct_dspace_refined); the D actions are true actions of exactly those vectors, one call of the
// action hook for all of them; and the D blocks of S and H come from these in R's precision (subspace.h
// update_dspace_refined).  The bound then has the D terms.  Cost: nD <= n_roots actions per rebuild, a rebuild in
// every iteration in which the limit deletes something -- which propose_rspace makes rarer by cutting the Q space
// below the limit (Refinement::dspace_slack).  reset_D / reset_D_max_Q_size stay outside the scope.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <vector>

#include "subspace.h"

namespace molpro::linalg::itsolv {

//! on: the refined mode; kappa <= 0: the default, 8; dspace: the consistent D space under max_size_qspace;
//! dspace_slack < 0: the default rule (Refinement::dspace_slack).
struct RefineOptions {
  bool on = false;
  double kappa = 8.0;
  bool dspace = false;
  int dspace_slack = -1;
};

// What a solve in the refined mode spent: actions on refined residuals, the iteration (from 1; 0: none) of the
// first, and the largest of the roots' last error bounds delta.
struct RefineStats {
  int refined_actions = 0;
  int first_refined_iteration = 0;
  double max_delta = 0;
  // rebuilds of the D space under the Q-space limit (in either mode), and the actions the consistent D space
  // spent on them (not in refined_actions)
  int dspace_rebuilds = 0;
  int dspace_actions = 0;
};

template <class R>
class Refinement {
 public:
  //! actions[k] = H parameters[k]
  using action_hook_type = std::function<void(const CVecRef<R>&, const VecRef<R>&)>;

  RefineOptions options;
  action_hook_type hook;  // set_refine_action's; the problem's action while solve() runs (HookScope)
  RefineStats stats;      // max_delta is filled by current_stats()
  std::vector<double> delta;  // the last bound of each root

  //! set_refine: the mode on or off, with every counter and the D-space option reset (the slack stays)
  void set(bool on, double kappa) {
    options.on = on;
    options.kappa = kappa > 0 ? kappa : 8.0;
    options.dspace = false;
    stats = RefineStats{};
    delta.clear();
  }
  void set_dspace(bool on) {
    if (on && !options.on) throw std::logic_error("refine_dspace: needs the refined mode (set_refine) first");
    options.dspace = on;
    stats.dspace_rebuilds = stats.dspace_actions = 0;
  }
  RefineStats current_stats() const {
    RefineStats s = stats;
    s.max_delta = 0;
    for (double d : delta) s.max_delta = std::max(s.max_delta, d);
    return s;
  }
  void require_hook() const {
    if (!hook)
      throw std::logic_error(
          "refine: needs the problem's action, which only solve() provides (not add_vector by hand) unless "
          "set_refine_action has given it (C API: IterativeSolverHbmSetRefineAction)");
  }

  // Puts `action` in the hook's place until the scope ends, then the caller's hook back: on every way out.
  struct HookScope {
    HookScope(action_hook_type& hook_, action_hook_type action) : hook(hook_), callers(std::move(hook_)) {
      hook = std::move(action);
    }
    ~HookScope() { hook = std::move(callers); }
    HookScope(const HookScope&) = delete;
    action_hook_type& hook;
    action_hook_type callers;
  };

  //! delta = u scale (sum_Q |c_j| |a_j| + sum_D |c_d| |a_d|) of the solution in row `root` of sol, with u = 2^-24
  //! the unit roundoff of the storage; scale puts it in the units of the solver's errors.
  static double bound(const subspace::Matrix<double>& sol, size_t root, const subspace::Dimensions& d,
                      const std::vector<double>& q_action_norms, const std::vector<double>& d_action_norms,
                      double scale) {
    constexpr double u = 5.9604644775390625e-08;  // 2^-24, the unit roundoff of binary32
    double delta = 0;
    for (size_t j = 0; j < d.nQ; ++j) delta += std::abs(sol(root, d.oQ + j)) * q_action_norms.at(j);
    for (size_t j = 0; j < d.nD; ++j) delta += std::abs(sol(root, d.oD + j)) * d_action_norms.at(j);
    delta *= u;
    delta *= scale;
    return delta;
  }
  //! whether an estimate is no longer accurate to 1 / kappa, or could be declared converged unverified
  bool triggers(double estimate, double delta, double threshold) const {
    return estimate <= std::max(options.kappa * delta, threshold + delta);
  }
  //! How far below max_size_qspace a rebuild of the consistent D space cuts the Q space.  0 is the reference's
  //! schedule: delete just enough, so a rebuild in every iteration once the Q space is full.  Unset
  //! (options.dspace_slack < 0) it is a rule in whole working sets (less than one spaces nothing): two per
  //! rebuild -- a rebuild every third iteration -- or one, whichever stays under a quarter of the limit; none
  //! where the limit is that tight, because there the smaller Q space costs more iterations than the rarer
  //! rounding saves.  The rule's constants were measured on one dense fixture
  //! (profiles/r14/q32_refined_dspace.md); a caller who knows better sets the value.  A value is cut to leave at
  //! least n_roots Q vectors.
  int dspace_slack(size_t n_roots, int max_size_qspace) const {
    if (max_size_qspace == std::numeric_limits<int>::max()) return 0;
    const size_t nr = n_roots, quarter4 = size_t(max_size_qspace);  // 4 x a quarter of the limit
    if (options.dspace_slack >= 0) return std::min(options.dspace_slack, std::max(0, max_size_qspace - int(nr)));
    return 4 * 2 * nr < quarter4 ? int(2 * nr) : 4 * nr < quarter4 ? int(nr) : 0;
  }
};

}  // namespace molpro::linalg::itsolv
