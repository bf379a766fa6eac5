// Davidson with the Q space stored in f32 (include/itsolv_hbm.h *_q32): the restated solver over
// R = hbm::Vec (f64), Q = hbm::VecF32, on the handlers of itsolv_hbm/hbm_handlers_f32.h.  The problems,
// the runner and the result layout are those of host/itsolv_capi.cpp.  The *_q32_refined entries run the
// same solver in its refined mode (itsolv_hbm/refine.h), the *_q32_refined_dspace entries with
// the consistent D space on top (set_refine_dspace), which admits max_size_qspace.
//
// This file lives outside host/ on purpose: every host/*.cpp is also built against the CPU emulation of
// the f64 C ABI, which has no mixed-precision entry points.
#include "../host/capi_problems.h"
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
