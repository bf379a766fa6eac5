"""The boundary of the refined f32 Q space under a Q-space limit (include/itsolv_hbm.h *_q32_refined_dspace,
ssp_q32_combine_widen, IterativeSolverHbmRefineDspaceStats), checked without a GPU: the libraries export the
new C ABI, the bindings declare it in sets of their own and keep loading a library that lacks it (the CPU
emulation of the f64 ABI), the solver with the option compiles for <Vec, VecF32, SparseP> and resolves the new
hook to the f32 overload, and the f64 headers and host/ still do not name the f32 side."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest

from test_q32_refined_boundary import makefile_cxxflags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "iterative-solver_amd")
LIBDIR = os.path.join(PKG, "lib")
EMUL = os.path.join(ROOT, "oracle", "build")

SSP_NAMES = ["ssp_q32_combine_widen"]
ITSOLV_NAMES = ["itsolv_davidson_dense_q32_refined_dspace", "itsolv_davidson_synth_q32_refined_dspace",
                "itsolv_q32_dspace_stats"]
RC_NAMES = ["IterativeSolverHbmRefineDspaceStats"]


def test_libraries_export_the_dspace_abi():
    so = ctypes.CDLL(os.path.join(LIBDIR, "libsubspace_hip.so"), mode=ctypes.RTLD_GLOBAL)
    assert not [n for n in SSP_NAMES if not hasattr(so, n)]
    it = ctypes.CDLL(os.path.join(LIBDIR, "libitsolv_hbm.so"))
    assert not [n for n in ITSOLV_NAMES + RC_NAMES if not hasattr(it, n)]


def test_bindings_list_and_declare_the_new_names():
    """The new names are optional at load, in sets of their own: the sets the earlier boundary tests pin stay
    what they were."""
    import iterative_solver
    import itsolv_hbm as ih
    import subspace_hip as sh

    assert set(SSP_NAMES) <= set(sh.EXPORTS) and set(SSP_NAMES) == set(sh.OPTIONAL_DSPACE)
    assert set(ITSOLV_NAMES) <= set(ih.EXPORTS) and set(ITSOLV_NAMES) == set(ih.OPTIONAL_DSPACE)
    assert set(RC_NAMES) == set(iterative_solver.DSPACE_SIG)
    assert not set(SSP_NAMES) & (set(sh.OPTIONAL) | set(sh.OPTIONAL_Q32) | set(sh.OPTIONAL_REFINED) | set(sh.OPTIONAL_ROWS) |
                                 set(sh.OPTIONAL_ROWS_Q))
    assert not set(ITSOLV_NAMES) & (set(ih.OPTIONAL) | set(ih.OPTIONAL_REFINED))
    assert not set(RC_NAMES) & (set(iterative_solver.REFINE_SIG) | set(iterative_solver.DEVICE_SIG))
    assert len(sh.load_library().ssp_q32_combine_widen.argtypes) == 8
    lib = ih.load_library()
    assert len(lib.itsolv_davidson_dense_q32_refined_dspace.argtypes) == 7
    assert len(lib.itsolv_davidson_synth_q32_refined_dspace.argtypes) == 7
    assert len(lib.itsolv_q32_dspace_stats.argtypes) == 2
    assert len(iterative_solver._load().IterativeSolverHbmRefineDspaceStats.argtypes) == 2
    # the stats call works without a device: nothing has run on this thread
    assert ih._dspace_stats() == {"dspace_rebuilds": 0, "dspace_actions": 0}
    assert ih._entry("itsolv_davidson_dense", True, True, True) is lib.itsolv_davidson_dense_q32_refined_dspace
    with pytest.raises(ValueError, match="refine_dspace.*refine=True"):
        ih._entry("itsolv_davidson_dense", True, False, True)
    with pytest.raises(ValueError, match="refine.*q32"):
        ih._entry("itsolv_davidson_dense", False, True, True)


EMUL_SCRIPT = r"""
import os, sys
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "iterative-solver_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import iterative_solver
import itsolv_hbm as ih
import subspace_hip as sh
EMUL = os.path.join(ROOT, "oracle", "build")
sh.LIB_PATH = os.path.join(EMUL, "libssp_emul.so")
ih.LIB_PATH = os.path.join(EMUL, "libitsolv_emul.so")
iterative_solver.LIB_PATH = os.path.join(EMUL, "libitsolv_emul.so")
lib = sh.load_library()
assert not hasattr(lib, "ssp_q32_combine_widen"), "the emulation is not expected to have the mixed entry points"
assert not hasattr(ih.load_library(), "itsolv_davidson_dense_q32_refined_dspace")
# host/ is built into the emulation too: the reverse-communication statistics are there
assert hasattr(iterative_solver._load(), "IterativeSolverHbmRefineDspaceStats")
with sh.Context(0) as ctx:
    x = ctx.upload(np.arange(8.0))
    calls = [lambda: ctx.q32_combine_widen(np.ones((1, 1)), [x], [x], [x]),
             lambda: ih.davidson_dense(ctx, np.eye(4), q32=True, refine=True, refine_dspace=True, nroots=1,
                                       max_size_qspace=2),
             lambda: ih.davidson_synthetic(ctx, 64, 0.1, 1, 1, q32=True, refine=True, refine_dspace=True,
                                           max_size_qspace=4)]
    for i, f in enumerate(calls):
        try:
            f()
        except sh.SspError as e:
            assert e.code == 7, (i, e)
        else:
            raise AssertionError(f"call {i} did not raise")
    for kw in (dict(refine_dspace=True), dict(q32=True, refine_dspace=True)):
        try:
            ih.davidson_dense(ctx, np.eye(4), nroots=1, **kw)
        except ValueError as e:
            assert "refine=True" in str(e)
        else:
            raise AssertionError("refine_dspace without refine did not raise")
    r = ih.davidson_dense(ctx, np.diag(np.arange(1.0, 9.0)), nroots=1, convergence_threshold=1e-8)
    assert r["converged"] and abs(r["eigenvalues"][0] - 1.0) < 1e-8 and "refine_dspace" not in r
print("ok")
"""


@pytest.mark.skipif(not os.path.exists(os.path.join(EMUL, "libssp_emul.so")), reason="needs `make -C oracle`")
def test_bindings_load_a_library_without_the_dspace_entry_points():
    r = subprocess.run([sys.executable, "-c", EMUL_SCRIPT, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


TU = r"""
#include "itsolv_hbm/hbm_handlers_f32.h"
#include "itsolv_hbm/problems.h"
#include "itsolv_hbm/solvers.h"
using namespace molpro::linalg;
template class itsolv::LinearEigensystemDavidson<hbm::Vec, hbm::VecF32, hbm::SparseP>;
using Solver = itsolv::LinearEigensystemDavidson<hbm::Vec, hbm::VecF32, hbm::SparseP>;
// the hook resolves to the f32 overload for the Q x Q handler of this pair, and to the default for Q = R
bool combine(itsolv::ArrayHandlers<hbm::Vec, hbm::VecF32, hbm::SparseP>& h, const itsolv::subspace::Matrix<double>& c,
             const std::vector<const hbm::VecF32*>& src, std::vector<hbm::VecF32>& out, const itsolv::VecRef<hbm::Vec>& w) {
  using array::fused_new_combinations_widened;
  return fused_new_combinations_widened(h.qq(), c, src, out, w);
}
bool combine_f64(itsolv::ArrayHandlers<hbm::Vec, hbm::Vec, hbm::SparseP>& h, const itsolv::subspace::Matrix<double>& c,
                 const std::vector<const hbm::Vec*>& src, std::vector<hbm::Vec>& out, const itsolv::VecRef<hbm::Vec>& w) {
  using array::fused_new_combinations_widened;
  return fused_new_combinations_widened(h.qq(), c, src, out, w);
}
bool solve(const itsolv::Problem<hbm::Vec, hbm::SparseP>& problem, std::vector<hbm::Vec>& x, std::vector<hbm::Vec>& a) {
  Solver solver(hbm::make_handlers_q32());
  solver.set_refine(true, 4.0);
  solver.set_refine_dspace(true);
  solver.set_max_size_qspace(12);
  solver.validate_refine();
  const bool ok = solver.solve(x, a, problem, true);
  return ok && solver.refine_dspace() && solver.dspace_rebuilds() >= 0 && solver.dspace_actions() >= 0;
}
void run(const itsolv::Problem<hbm::Vec, hbm::SparseP>& problem, const itsolv_options& o, itsolv_result& out) {
  const itsolv::RefineOptions refine{true, 0, true};  // kappa <= 0: the default; with the consistent D space
  itsolv::RefineStats stats;
  itsolv::problems::run_davidson<hbm::Vec, hbm::VecF32, hbm::SparseP>(hbm::make_handlers_q32(), problem, {}, {}, o, out,
                                                                     {}, {}, &refine, &stats);
}
"""


def test_refined_dspace_davidson_compiles_with_an_f32_q_space():
    flags = makefile_cxxflags()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "q32_refined_dspace_tu.cpp")
        with open(src, "w") as f:
            f.write(TU)
        r = subprocess.run([os.environ.get("CXX", "g++")] + flags + ["-fsyntax-only", src], cwd=PKG, capture_output=True,
                           text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]


def test_f64_headers_and_host_name_the_f32_side_only_through_the_face():
    inc = os.path.join(PKG, "include", "itsolv_hbm")
    for name in os.listdir(inc):
        if name in ("hbm_vec_f32.h", "hbm_handlers_f32.h"):
            continue
        text = open(os.path.join(inc, name)).read()
        assert "ssp_q32_" not in text and "hbm_handlers_f32.h" not in text and "hbm_vec_f32.h" not in text, name
    assert "ssp_q32_combine_widen" in open(os.path.join(inc, "hbm_handlers_f32.h")).read()
    for name in os.listdir(os.path.join(PKG, "host")):  # host/ is also built against the f64 emulation
        text = open(os.path.join(PKG, "host", name)).read()
        assert "ssp_q32_" not in text and "_f32" not in text, name
