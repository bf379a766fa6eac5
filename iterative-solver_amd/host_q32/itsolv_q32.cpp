// Davidson with the Q space stored in f32 (include/itsolv_hbm.h *_q32): the restated solver over
// R = hbm::Vec (f64), Q = hbm::VecF32, on the handlers of itsolv_hbm/hbm_handlers_f32.h.  The problems,
// the runner and the result layout are those of host/itsolv_capi.cpp.  The *_q32_refined entries run the
// same solver in its refined mode (itsolv_hbm/solvers.h set_refine), the *_q32_refined_dspace entries with
// the consistent D space on top (set_refine_dspace), which admits max_size_qspace.
//
// This file lives outside host/ on purpose: every host/*.cpp is also built against the CPU emulation of
// the f64 C ABI, which has no mixed-precision entry points.
#include "../host/capi_problems.h"
#include "itsolv_hbm/hbm_handlers_f32.h"

using namespace itsolv_capi;
using molpro::linalg::hbm::VecF32;

namespace {

thread_local pr::RefineStats g_refine_stats;  // itsolv_q32_refine_stats()

// refine: null for the plain f32 Q space; else the refined mode (kappa <= 0: the default).
int synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt, const double* kappa,
              itsolv_result* out, double* solutions_out, bool dspace = false) {
  return guarded([&] {
    auto dev = borrow(ctx);
    const auto o = opts_or_default(opt);
    SyntheticProblem problem(dev, spec_of(n, spec));
    std::memset(out, 0, sizeof(*out));
    pr::run_davidson<Vec, VecF32, SparseP>(
        molpro::linalg::hbm::make_handlers_q32(), problem, [&] { return zero_vec(dev, n); },
        [&](const Vec& x, double e) { return residual_norm(problem, dev, x, e); }, o, *out,
        [&](size_t r, const Vec& x) {
          if (!solutions_out) return;
          auto v = x.local_values();
          std::memcpy(solutions_out + r * v.size(), v.data(), v.size() * sizeof(double));
        },
        residual_norms_batch(problem, dev, n), kappa, kappa ? &g_refine_stats : nullptr, dspace);
  });
}

int dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, const double* kappa,
              itsolv_result* out, double* solutions_out, bool dspace = false) {
  return guarded([&] {
    auto dev = borrow(ctx);
    const auto o = opts_or_default(opt);
    DenseProblem problem(dev, h, n);
    std::memset(out, 0, sizeof(*out));
    pr::run_davidson<Vec, VecF32, SparseP>(
        molpro::linalg::hbm::make_handlers_q32(), problem, [&] { return zero_vec(dev, n); },
        [&](const Vec& x, double e) { return residual_norm(problem, dev, x, e); }, o, *out,
        [&](size_t r, const Vec& x) {
          if (!solutions_out) return;
          auto v = x.local_values();
          std::memcpy(solutions_out + r * n, v.data(), n * sizeof(double));
        },
        {}, kappa, kappa ? &g_refine_stats : nullptr, dspace);
  });
}

double kappa_of(const itsolv_q32_refine* r) { return r ? r->kappa : 0.0; }

}  // namespace

extern "C" {

int itsolv_davidson_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                              itsolv_result* out, double* solutions_out) {
  return synth_q32(ctx, n, spec, opt, nullptr, out, solutions_out);
}

int itsolv_davidson_dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                              double* solutions_out) {
  return dense_q32(ctx, h, n, opt, nullptr, out, solutions_out);
}

int itsolv_davidson_synth_q32_refined(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                                      const itsolv_q32_refine* refine, itsolv_result* out, double* solutions_out) {
  g_refine_stats = pr::RefineStats{};
  const double kappa = kappa_of(refine);
  return synth_q32(ctx, n, spec, opt, &kappa, out, solutions_out);
}

int itsolv_davidson_dense_q32_refined(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt,
                                      const itsolv_q32_refine* refine, itsolv_result* out, double* solutions_out) {
  g_refine_stats = pr::RefineStats{};
  const double kappa = kappa_of(refine);
  return dense_q32(ctx, h, n, opt, &kappa, out, solutions_out);
}

int itsolv_davidson_synth_q32_refined_dspace(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                                             const itsolv_q32_refine* refine, itsolv_result* out,
                                             double* solutions_out) {
  g_refine_stats = pr::RefineStats{};
  const double kappa = kappa_of(refine);
  return synth_q32(ctx, n, spec, opt, &kappa, out, solutions_out, true);
}

int itsolv_davidson_dense_q32_refined_dspace(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt,
                                             const itsolv_q32_refine* refine, itsolv_result* out,
                                             double* solutions_out) {
  g_refine_stats = pr::RefineStats{};
  const double kappa = kappa_of(refine);
  return dense_q32(ctx, h, n, opt, &kappa, out, solutions_out, true);
}

// Linear equations over the f32 Q space: plain (the right-hand sides stored rounded with the Q space; meaningful
// down to about 1e-6) and refined (f64 twins of the right-hand sides, refined residuals: f64 thresholds).
int itsolv_linear_equations_dense_q32(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                      const itsolv_options* opt, itsolv_result* out, double* x_out) {
  return guarded([&] {
    linear_equations_dense<VecF32>(ctx, a, n, rhs, nrhs, molpro::linalg::hbm::make_handlers_q32(), opt, out, x_out);
  });
}

int itsolv_linear_equations_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs,
                                      unsigned long long rhs_seed, const itsolv_options* opt, itsolv_result* out,
                                      double* x_out) {
  return guarded([&] {
    linear_equations_synth<VecF32>(ctx, n, spec, nrhs, rhs_seed, molpro::linalg::hbm::make_handlers_q32(), opt, out,
                                   x_out);
  });
}

int itsolv_linear_equations_dense_q32_refined(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                              const itsolv_options* opt, const itsolv_q32_refine* refine,
                                              itsolv_result* out, double* x_out) {
  g_refine_stats = pr::RefineStats{};
  const double kappa = kappa_of(refine);
  return guarded([&] {
    linear_equations_dense<VecF32>(ctx, a, n, rhs, nrhs, molpro::linalg::hbm::make_handlers_q32(), opt, out, x_out,
                                   &kappa, &g_refine_stats);
  });
}

int itsolv_linear_equations_synth_q32_refined(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs,
                                              unsigned long long rhs_seed, const itsolv_options* opt,
                                              const itsolv_q32_refine* refine, itsolv_result* out, double* x_out) {
  g_refine_stats = pr::RefineStats{};
  const double kappa = kappa_of(refine);
  return guarded([&] {
    linear_equations_synth<VecF32>(ctx, n, spec, nrhs, rhs_seed, molpro::linalg::hbm::make_handlers_q32(), opt, out,
                                   x_out, &kappa, &g_refine_stats);
  });
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
