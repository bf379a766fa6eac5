// Davidson with the Q space stored in f32 (include/itsolv_hbm.h *_q32): the restated solver over
// R = hbm::Vec (f64), Q = hbm::VecF32, on the handlers of itsolv_hbm/hbm_handlers_f32.h.  The problems,
// the runner and the result layout are those of host/itsolv_capi.cpp.
//
// This file lives outside host/ on purpose: every host/*.cpp is also built against the CPU emulation of
// the f64 C ABI, which has no mixed-precision entry points.
#include "../host/capi_problems.h"
#include "itsolv_hbm/hbm_handlers_f32.h"

using namespace itsolv_capi;
using molpro::linalg::hbm::VecF32;

extern "C" {

int itsolv_davidson_synth_q32(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                              itsolv_result* out, double* solutions_out) {
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
        residual_norms_batch(problem, dev, n));
  });
}

int itsolv_davidson_dense_q32(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                              double* solutions_out) {
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
        });
  });
}

}  // extern "C"
