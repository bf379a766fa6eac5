"""The boundary of the linear equations over an f32 Q space (include/subspace_hip.h ssp_mx_rhs_residual_norms;
include/itsolv_hbm.h itsolv_linear_equations_*), checked without a GPU: the libraries export the new C ABI, the
bindings declare it in optional sets of their own and keep loading a library that lacks it (the CPU emulation of
the f64 ABI), LinearEquationsDavidson<Vec, VecF32, SparseP> with set_refine compiles, the fused-residual hook
resolves to the f32 overloads for the q32 handler set only, and itsolv_linear_equations_synth -- f64, so part of
the emulation too -- solves a sharded-size problem there."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "iterative-solver_amd")
LIBDIR = os.path.join(PKG, "lib")
EMUL = os.path.join(ROOT, "oracle", "build")

SSP_NAMES = ["ssp_mx_rhs_residual_norms"]
ITSOLV_Q32 = ["itsolv_linear_equations_dense_q32", "itsolv_linear_equations_synth_q32",
              "itsolv_linear_equations_dense_q32_refined", "itsolv_linear_equations_synth_q32_refined"]
ITSOLV_F64 = ["itsolv_linear_equations_synth"]


def test_libraries_export_the_new_abi():
    so = ctypes.CDLL(os.path.join(LIBDIR, "libsubspace_hip.so"), mode=ctypes.RTLD_GLOBAL)
    assert not [n for n in SSP_NAMES if not hasattr(so, n)]
    it = ctypes.CDLL(os.path.join(LIBDIR, "libitsolv_hbm.so"))
    assert not [n for n in ITSOLV_Q32 + ITSOLV_F64 if not hasattr(it, n)]


def test_bindings_list_and_declare_the_new_names():
    """The new names are optional at load, in sets of their own (OPTIONAL_LINEQ): the other sets stay what the
    existing boundary tests pin."""
    import itsolv_hbm as ih
    import subspace_hip as sh

    assert set(SSP_NAMES) <= set(sh.EXPORTS) and set(SSP_NAMES) == set(sh.OPTIONAL_LINEQ)
    assert set(ITSOLV_Q32 + ITSOLV_F64) <= set(ih.EXPORTS) and set(ITSOLV_Q32) == set(ih.OPTIONAL_LINEQ)
    others = (set(sh.OPTIONAL) | set(sh.OPTIONAL_Q32) | set(sh.OPTIONAL_REFINED) | set(sh.OPTIONAL_ROWS) |
              set(sh.OPTIONAL_ROWS_Q) | set(sh.OPTIONAL_DSPACE))
    assert not set(SSP_NAMES) & others
    assert not set(ITSOLV_Q32 + ITSOLV_F64) & (set(ih.OPTIONAL) | set(ih.OPTIONAL_REFINED) | set(ih.OPTIONAL_DSPACE))
    assert len(sh.load_library().ssp_mx_rhs_residual_norms.argtypes) == 9
    lib = ih.load_library()
    assert len(lib.itsolv_linear_equations_synth.argtypes) == 8
    assert len(lib.itsolv_linear_equations_dense_q32.argtypes) == 8
    assert len(lib.itsolv_linear_equations_synth_q32.argtypes) == 8
    assert len(lib.itsolv_linear_equations_dense_q32_refined.argtypes) == 9
    assert len(lib.itsolv_linear_equations_synth_q32_refined.argtypes) == 9
    with pytest.raises(ValueError, match="refine.*q32"):
        ih._entry("itsolv_linear_equations_dense", False, True)


EMUL_SCRIPT = r"""
import os, sys
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "iterative-solver_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import itsolv_hbm as ih
import oracle
import subspace_hip as sh
EMUL = os.path.join(ROOT, "oracle", "build")
sh.LIB_PATH = os.path.join(EMUL, "libssp_emul.so")
ih.LIB_PATH = os.path.join(EMUL, "libitsolv_emul.so")
lib = sh.load_library()
assert not hasattr(lib, "ssp_mx_rhs_residual_norms"), "the emulation is not expected to have the mixed entry points"
assert not hasattr(ih.load_library(), "itsolv_linear_equations_dense_q32")
EPS = float(np.finfo(np.float64).eps)
with sh.Context(0) as ctx:
    y = ctx.upload(np.arange(5.0))
    a, b = np.diag(np.arange(1.0, 5.0)), np.ones((1, 4))
    calls = [lambda: ctx.mx_rhs_residual_norms([y], [1.0], [y]),
             lambda: ih.linear_equations_dense(ctx, a, b, q32=True),
             lambda: ih.linear_equations_dense(ctx, a, b, q32=True, refine=True, kappa=4.0),
             lambda: ih.linear_equations_synth(ctx, 64, 0.1, 1, 1, 2, 5, q32=True),
             lambda: ih.linear_equations_synth(ctx, 64, 0.1, 1, 1, 2, 5, q32=True, refine=True)]
    for i, f in enumerate(calls):
        try:
            f()
        except sh.SspError as e:
            assert e.code == 7, (i, e)
        else:
            raise AssertionError(f"call {i} did not raise")
    try:
        ih.linear_equations_dense(ctx, a, b, refine=True)
    except ValueError as e:
        assert "q32" in str(e)
    else:
        raise AssertionError("refine without q32 did not raise")
    r = ih.linear_equations_dense(ctx, a, b, convergence_threshold=1e-10)
    assert r["converged"] and np.allclose(r["x"][0], 1 / np.arange(1.0, 5.0)) and "refine" not in r

    # the f64 synthetic entry: n = 10007, rank 2, 3 right-hand sides at 1e-10
    n, rho, rank, seed, nrhs, rhs_seed, thr = 10007, 0.5, 2, 3, 3, 17, 1e-10
    r = ih.linear_equations_synth(ctx, n, rho, rank, seed, nrhs, rhs_seed, convergence_threshold=thr, max_iter=100)
    assert r["converged"], (r["iterations"], r["errors"])
    norm2 = n + rank * rho * n  # |H|_2 <= max d + rho |sum_l u_l u_l^T|_2 <= n + rho rank n
    for k in range(nrhs):
        b_k = oracle.random_vector(n, rhs_seed, k)
        x_k = r["x"][k]
        res = np.linalg.norm(oracle.synthetic_action(x_k, rho, rank, seed) - b_k) / np.linalg.norm(b_k)
        # both recomputations round: n eps (|H|_2 |x| + |b|) / |b| each
        recompute = n * EPS * (norm2 * np.linalg.norm(x_k) + np.linalg.norm(b_k)) / np.linalg.norm(b_k)
        print(k, r["residual_norms"][k], res, recompute)
        assert abs(r["residual_norms"][k] - res) <= 2 * recompute, (k, r["residual_norms"][k], res, recompute)
        assert res <= thr + recompute
print("ok")
"""


@pytest.mark.skipif(not os.path.exists(os.path.join(EMUL, "libssp_emul.so")), reason="needs `make -C oracle`")
def test_emulation_loads_without_the_new_entry_points_and_solves_the_synthetic_equations():
    r = subprocess.run([sys.executable, "-c", EMUL_SCRIPT, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


TU = r"""
#include "itsolv_hbm/hbm_handlers_f32.h"
#include "itsolv_hbm/problems.h"
#include "itsolv_hbm/solvers.h"
using namespace molpro::linalg;
template class itsolv::LinearEquationsDavidson<hbm::Vec, hbm::VecF32, hbm::SparseP>;
using Solver = itsolv::LinearEquationsDavidson<hbm::Vec, hbm::VecF32, hbm::SparseP>;
// the hook resolves to the f32 overloads for the R x Q handler of this pair (stored right-hand sides and their
// f64 twins), and to the default for Q = R
bool stored(itsolv::ArrayHandlers<hbm::Vec, hbm::VecF32, hbm::SparseP>& h, const itsolv::CVecRef<hbm::VecF32>& b,
            const itsolv::VecRef<hbm::Vec>& y, std::vector<double>& n2) {
  using array::fused_rhs_residual_norms;
  return fused_rhs_residual_norms(h.rq(), std::vector<double>(y.size(), 1.0), b, y, n2);
}
bool twins(itsolv::ArrayHandlers<hbm::Vec, hbm::VecF32, hbm::SparseP>& h, const itsolv::CVecRef<hbm::Vec>& b,
           const itsolv::VecRef<hbm::Vec>& y, std::vector<double>& n2) {
  using array::fused_rhs_residual_norms;
  return fused_rhs_residual_norms(h.rq(), std::vector<double>(y.size(), 1.0), b, y, n2);
}
bool f64(itsolv::ArrayHandlers<hbm::Vec, hbm::Vec, hbm::SparseP>& h, const itsolv::CVecRef<hbm::Vec>& b,
         const itsolv::VecRef<hbm::Vec>& y, std::vector<double>& n2) {
  using array::fused_rhs_residual_norms;
  return fused_rhs_residual_norms(h.rq(), std::vector<double>(y.size(), 1.0), b, y, n2);
}
bool solve(const itsolv::Problem<hbm::Vec, hbm::SparseP>& problem, std::vector<hbm::Vec>& b, std::vector<hbm::Vec>& x,
           std::vector<hbm::Vec>& a) {
  Solver solver(hbm::make_handlers_q32());
  solver.set_refine(true, 4.0);
  solver.add_equations(b);
  const bool ok = solver.solve(x, a, problem, true);
  return ok && solver.refined_actions() >= 0 && solver.xspace().rhs_r().size() == b.size();
}
void run(const itsolv::Problem<hbm::Vec, hbm::SparseP>& problem, std::vector<hbm::Vec>& b, const itsolv_options& o,
         itsolv_result& out) {
  const itsolv::RefineOptions refine{true, 0};  // kappa <= 0: the default
  itsolv::RefineStats stats;
  itsolv::problems::run_linear_equations<hbm::Vec, hbm::VecF32, hbm::SparseP>(hbm::make_handlers_q32(), problem, {}, b, {},
                                                                             o, out, {}, &refine, &stats);
}
"""


def makefile_cxxflags():
    out = subprocess.run(["make", "-pn", "-C", PKG, "clean"], capture_output=True, text=True, timeout=120).stdout
    for line in out.splitlines():
        if line.startswith("CXXFLAGS := ") or line.startswith("CXXFLAGS = "):
            return line.split("=", 1)[1].split()
    raise AssertionError("CXXFLAGS not found in the Makefile's database")


def test_refined_linear_equations_compile_with_an_f32_q_space():
    flags = makefile_cxxflags()
    assert "-std=c++17" in flags
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "q32_lineq_tu.cpp")
        with open(src, "w") as f:
            f.write(TU)
        r = subprocess.run([os.environ.get("CXX", "g++")] + flags + ["-fsyntax-only", src], cwd=PKG, capture_output=True,
                           text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]


def test_f64_headers_and_host_sources_do_not_name_the_mixed_entry_point():
    """The hook is type-generic: only hbm_handlers_f32.h names the C entry point, so that host/ still builds
    against the emulation of the f64 ABI."""
    inc = os.path.join(PKG, "include", "itsolv_hbm")
    for name in os.listdir(inc):
        text = open(os.path.join(inc, name)).read()
        assert ("ssp_mx_rhs_residual_norms" in text) == (name == "hbm_handlers_f32.h"), name
    for name in os.listdir(os.path.join(PKG, "host")):
        assert "ssp_mx_rhs_residual_norms" not in open(os.path.join(PKG, "host", name)).read(), name
