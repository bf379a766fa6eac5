// libitsolv_hbm.so: the restated solvers (include/itsolv_hbm/solvers.h) over HBM vectors and the
// HIP handlers, behind the C ABI of include/itsolv_hbm.h.  Problem actions run on the device
// (sspx_* kernels), so R, Q and the diagonals never leave HBM during a solve.
#include "capi_problems.h"

using namespace itsolv_capi;

extern "C" {

const char* itsolv_last_error(void) { return g_error.c_str(); }

void itsolv_default_options(itsolv_options* opt) { pr::default_options(opt); }

int itsolv_davidson_synthetic(ssp_ctx* ctx, size_t n, double rho, int rank, unsigned long long seed,
                              const itsolv_options* opt, itsolv_result* out, double* solutions_out) {
  const sspx_synth s{rho, rank, seed, SSPX_DIAG_LINEAR, 0.0, 1.0};
  return itsolv_davidson_synth(ctx, n, &s, opt, out, solutions_out);
}

int itsolv_davidson_synth(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt,
                          itsolv_result* out, double* solutions_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    const auto o = opts_or_default(opt);
    SyntheticProblem problem(dev, spec_of(n, spec));
    std::memset(out, 0, sizeof(*out));
    pr::run_davidson<Vec, Vec, SparseP>(
        molpro::linalg::hbm::make_handlers(), problem, [&] { return zero_vec(dev, n); },
        [&](const Vec& x, double e) { return residual_norm(problem, dev, x, e); }, o, *out,
        emit_local(solutions_out), residual_norms_batch(problem, dev, n));
  });
}

int itsolv_davidson_dense(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                          double* solutions_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    const auto o = opts_or_default(opt);
    DenseProblem problem(dev, h, n);
    std::memset(out, 0, sizeof(*out));
    pr::run_davidson<Vec, Vec, SparseP>(
        molpro::linalg::hbm::make_handlers(), problem, [&] { return zero_vec(dev, n); },
        [&](const Vec& x, double e) { return residual_norm(problem, dev, x, e); }, o, *out,
        emit_local(solutions_out));  // (a dense problem is on one rank: the local part is the whole)
  });
}

int itsolv_diis_synthetic(ssp_ctx* ctx, size_t n, double rho, int rank, unsigned long long seed,
                          const itsolv_options* opt, itsolv_result* out, double* x_out) {
  const sspx_synth s{rho, rank, seed, SSPX_DIAG_LINEAR, 0.0, 1.0};
  return itsolv_diis_synth(ctx, n, &s, opt, out, x_out);
}

int itsolv_diis_synth(ssp_ctx* ctx, size_t n, const sspx_synth* spec, const itsolv_options* opt, itsolv_result* out,
                      double* x_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    const auto o = opts_or_default(opt);
    SyntheticProblem problem(dev, spec_of(n, spec));
    std::memset(out, 0, sizeof(*out));
    pr::run_diis<Vec, Vec, SparseP>(
        molpro::linalg::hbm::make_handlers(), problem, [&] { return zero_vec(dev, n); },
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
        });
  });
}

int itsolv_linear_equations_dense(ssp_ctx* ctx, const double* a, size_t n, const double* rhs, int nrhs,
                                  const itsolv_options* opt, itsolv_result* out, double* x_out) {
  return guarded([&] {
    linear_equations_dense<Vec>(ctx, a, n, rhs, nrhs, molpro::linalg::hbm::make_handlers(), opt, out, x_out);
  });
}

int itsolv_linear_equations_synth(ssp_ctx* ctx, size_t n, const sspx_synth* spec, int nrhs, unsigned long long rhs_seed,
                                  const itsolv_options* opt, itsolv_result* out, double* x_out) {
  return guarded([&] {
    linear_equations_synth<Vec>(ctx, n, spec, nrhs, rhs_seed, molpro::linalg::hbm::make_handlers(), opt, out, x_out);
  });
}

int itsolv_optimize_dense(ssp_ctx* ctx, const double* h, size_t n, int algorithm, const itsolv_options* opt,
                          itsolv_result* out, double* x_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    const auto o = opts_or_default(opt);
    RayleighProblem problem(dev, h, n);
    std::memset(out, 0, sizeof(*out));
    pr::run_optimize<Vec, Vec, SparseP>(
        molpro::linalg::hbm::make_handlers(), problem, [&] { return zero_vec(dev, n); },
        [&](Vec& x) {
          const size_t i0 = 0;
          const double one = 1.0;
          check(ssp_sparse_copy(x.ctx(), x.data_wo(), x.local_size(), x.offset(), &i0, &one, 1), "ssp_sparse_copy");
        },
        algorithm, o, *out,
        [&](const Vec& x) {
          if (!x_out) return;
          auto v = x.local_values();
          std::memcpy(x_out, v.data(), v.size() * sizeof(double));
        });
  });
}

int itsolv_diis_dense(ssp_ctx* ctx, const double* h, size_t n, const itsolv_options* opt, itsolv_result* out,
                      double* x_out) {
  return guarded([&] {
    auto dev = borrow(ctx);
    const auto o = opts_or_default(opt);
    DenseProblem problem(dev, h, n);
    std::memset(out, 0, sizeof(*out));
    pr::run_diis<Vec, Vec, SparseP>(
        molpro::linalg::hbm::make_handlers(), problem, [&] { return zero_vec(dev, n); },
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
        });
  });
}

}  // extern "C"
