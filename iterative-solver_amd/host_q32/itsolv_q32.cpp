// Davidson with the Q space stored in f32 (include/itsolv_hbm.h *_q32): the restated solver over
// R = hbm::Vec (f64), Q = hbm::VecF32, on the handlers of itsolv_hbm/hbm_handlers_f32.h.  The problems,
// the runner and the result layout are those of host/itsolv_capi.cpp.  The *_q32_refined entries run the
// same solver in its refined mode (itsolv_hbm/refine.h), the *_q32_refined_dspace entries with
// the consistent D space on top (set_refine_dspace), which admits max_size_qspace.  The itsolv_diis_*_q32 entries
// run NonLinearEquationsDIISDifferences (itsolv_hbm/diis_differences.h) over the same handlers.
//
// This file lives outside host/ on purpose: every host/*.cpp is also built against the CPU emulation of
// the f64 C ABI, which has no mixed-precision entry points.
#include "../host/capi_problems.h"
#include "itsolv_hbm/diis_differences.h"
#include "itsolv_hbm/hbm_handlers_f32.h"

using namespace itsolv_capi;
using molpro::linalg::hbm::VecF32;

namespace {

thread_local RefineStats g_refine_stats;  // itsolv_q32_refine_stats(), itsolv_q32_dspace_stats()

const RefineOptions kPlain{};  // the plain f32 Q space

// The options of a *_refined entry (kappa <= 0, or no itsolv_q32_refine: the default), with this thread's
// statistics reset for its solve.
RefineOptions refined(const itsolv_q32_refine* r, bool dspace = false) {
  g_refine_stats = RefineStats{};
  return RefineOptions{true, r ? r->kappa : 0.0, dspace, -1};
}
RefineStats* stats_of(const RefineOptions& refine) { return refine.on ? &g_refine_stats : nullptr; }

template <class PROB>
void davidson_q32(const std::shared_ptr<Device>& dev, const PROB& problem, size_t n, const itsolv_options* opt,
                  const RefineOptions& refine, itsolv_result* out, double* solutions_out,
                  const pr::ResidualNormsBatch<Vec>& norms_batch) {
  std::memset(out, 0, sizeof(*out));
  pr::run_davidson<Vec, VecF32, SparseP>(
      molpro::linalg::hbm::make_handlers_q32(), problem, [&] { return zero_vec(dev, n); },
      [&](const Vec& x, double e) { return residual_norm(problem, dev, x, e); }, opts_or_default(opt), *out,
      emit_local(solutions_out), norms_batch, &refine, stats_of(refine));
}

int synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt, const RefineOptions& refine,
              itsolv_result* out, double* solutions_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    SyntheticProblem problem(dev, spec_of(n, spec));
    davidson_q32(dev, problem, n, opt, refine, out, solutions_out, residual_norms_batch(problem, dev, n));
  });
}

int dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, const RefineOptions& refine,
              itsolv_result* out, double* solutions_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    DenseProblem problem(dev, h, n);
    davidson_q32(dev, problem, n, opt, refine, out, solutions_out, {});
  });
}

int lineq_dense_q32(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs, const itsolv_options* opt,
                    const RefineOptions& refine, itsolv_result* out, double* x_out) {
  return guarded([&] {
    linear_equations_dense<VecF32>(ctx, a, n, rhs, nrhs, molpro::linalg::hbm::make_handlers_q32(), opt, out, x_out,
                                   &refine, stats_of(refine));
  });
}

int lineq_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs, unsigned long long rhs_seed,
                    const itsolv_options* opt, const RefineOptions& refine, itsolv_result* out, double* x_out) {
  return guarded([&] {
    linear_equations_synth<VecF32>(ctx, n, spec, nrhs, rhs_seed, molpro::linalg::hbm::make_handlers_q32(), opt, out,
                                   x_out, &refine, stats_of(refine));
  });
}

struct DiisStats {
  int points = 0, pairs = 0;
  size_t history_bytes = 0;
};
thread_local DiisStats g_diis_stats;  // itsolv_q32_diis_stats()

size_t arena_in_use(ssp_ctx* ctx) {
  size_t in_use = 0, cached = 0;
  check(ssp_memory_stats(ctx, &in_use, &cached), "ssp_memory_stats");
  return in_use;
}

template <class PROB>
void diis_q32(const std::shared_ptr<Device>& dev, const PROB& problem, size_t n, const itsolv_options* opt,
              itsolv_result* out, double* x_out) {
  using Solver = molpro::linalg::itsolv::NonLinearEquationsDIISDifferences<Vec, VecF32, SparseP>;
  if (dev->nranks() > 1)
    throw std::invalid_argument("itsolv_diis_*_q32: not available on a context with more than one rank");
  const auto o = opts_or_default(opt);
  if (o.max_p > 0) throw std::invalid_argument("itsolv_diis_*_q32: max_p: a P space is not supported");
  std::memset(out, 0, sizeof(*out));
  g_diis_stats = DiisStats{};
  // the history's bytes: what the arena holds when the solve ends, less what it held before and the runner's
  // own two vectors
  const size_t before = arena_in_use(dev->ctx());
  size_t vec_bytes = 0;
  {
    const Vec probe = zero_vec(dev, n);
    vec_bytes = arena_in_use(dev->ctx()) - before;
  }
  pr::run_diis_with<Solver, Vec, VecF32, SparseP>(
      molpro::linalg::hbm::make_handlers_q32(), problem, [&] { return zero_vec(dev, n); },
      [&](Vec& x) {
        const size_t i0 = 0;
        const double one = 1.0;
        check(ssp_sparse_copy(x.ctx(), x.data_wo(), x.local_size(), x.offset(), &i0, &one, 1), "ssp_sparse_copy");
      },
      o, *out,
      [&](const Vec& x) {
        if (!x_out) return;
        auto v = x.local_values();
        std::memcpy(x_out, v.data(), v.size() * sizeof(double));
      },
      [&](const Solver& solver) {
        g_diis_stats.points = int(solver.size());
        g_diis_stats.pairs = int(solver.difference_pairs());
        const size_t now = arena_in_use(dev->ctx());
        g_diis_stats.history_bytes = now > before + 2 * vec_bytes ? now - before - 2 * vec_bytes : 0;
      });
}

}  // namespace

extern "C" {

int itsolv_davidson_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                              itsolv_result* out, double* solutions_out) {
  return synth_q32(ctx, n, spec, opt, kPlain, out, solutions_out);
}

int itsolv_davidson_dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                              double* solutions_out) {
  return dense_q32(ctx, h, n, opt, kPlain, out, solutions_out);
}

int itsolv_davidson_synth_q32_refined(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                                      const itsolv_q32_refine* refine, itsolv_result* out, double* solutions_out) {
  return synth_q32(ctx, n, spec, opt, refined(refine), out, solutions_out);
}

int itsolv_davidson_dense_q32_refined(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt,
                                      const itsolv_q32_refine* refine, itsolv_result* out, double* solutions_out) {
  return dense_q32(ctx, h, n, opt, refined(refine), out, solutions_out);
}

int itsolv_davidson_synth_q32_refined_dspace(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                                             const itsolv_q32_refine* refine, itsolv_result* out,
                                             double* solutions_out) {
  return synth_q32(ctx, n, spec, opt, refined(refine, true), out, solutions_out);
}

int itsolv_davidson_dense_q32_refined_dspace(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt,
                                             const itsolv_q32_refine* refine, itsolv_result* out,
                                             double* solutions_out) {
  return dense_q32(ctx, h, n, opt, refined(refine, true), out, solutions_out);
}

// Linear equations over the f32 Q space: plain (the right-hand sides stored rounded with the Q space; meaningful
// down to about 1e-6) and refined (f64 twins of the right-hand sides, refined residuals: f64 thresholds).
int itsolv_linear_equations_dense_q32(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                      const itsolv_options* opt, itsolv_result* out, double* x_out) {
  return lineq_dense_q32(ctx, a, n, rhs, nrhs, opt, kPlain, out, x_out);
}

int itsolv_linear_equations_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs,
                                      unsigned long long rhs_seed, const itsolv_options* opt, itsolv_result* out,
                                      double* x_out) {
  return lineq_synth_q32(ctx, n, spec, nrhs, rhs_seed, opt, kPlain, out, x_out);
}

int itsolv_linear_equations_dense_q32_refined(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                              const itsolv_options* opt, const itsolv_q32_refine* refine,
                                              itsolv_result* out, double* x_out) {
  return lineq_dense_q32(ctx, a, n, rhs, nrhs, opt, refined(refine), out, x_out);
}

int itsolv_linear_equations_synth_q32_refined(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs,
                                              unsigned long long rhs_seed, const itsolv_options* opt,
                                              const itsolv_q32_refine* refine, itsolv_result* out, double* x_out) {
  return lineq_synth_q32(ctx, n, spec, nrhs, rhs_seed, opt, refined(refine), out, x_out);
}

// DIIS with its history as f32 differences behind f64 anchors (itsolv_hbm/diis_differences.h).
int itsolv_diis_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt, itsolv_result* out,
                          double* x_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    SyntheticProblem problem(dev, spec_of(n, spec));
    diis_q32(dev, problem, n, opt, out, x_out);
  });
}

int itsolv_diis_dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                          double* x_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    DenseProblem problem(dev, h, n);
    diis_q32(dev, problem, n, opt, out, x_out);
  });
}

int itsolv_q32_diis_stats(int* points, int* pairs, size_t* history_bytes) {
  if (points) *points = g_diis_stats.points;
  if (pairs) *pairs = g_diis_stats.pairs;
  if (history_bytes) *history_bytes = g_diis_stats.history_bytes;
  return 0;
}

int itsolv_q32_dspace_stats(int* rebuilds, int* actions) {
  if (rebuilds) *rebuilds = g_refine_stats.dspace_rebuilds;
  if (actions) *actions = g_refine_stats.dspace_actions;
  return 0;
}

int itsolv_q32_refine_stats(int* refined_actions, int* first_refined_iteration, double* max_delta) {
  if (refined_actions) *refined_actions = g_refine_stats.refined_actions;
  if (first_refined_iteration) *first_refined_iteration = g_refine_stats.first_refined_iteration;
  if (max_delta) *max_delta = g_refine_stats.max_delta;
  return 0;
}

}  // extern "C"
