"""The boundary of the f32 Q space and the refined mode in the reverse-communication API, checked without a GPU:
the libraries export the new C ABI (ssp_rows_export_quantised; IterativeSolverHbmSetRefineAction,
RefineStatistics, QStorage, Quantise[Device]), the bindings declare the new names in sets of their own and keep
loading a library that lacks them (the CPU emulation of the f64 ABI), and host/ still names nothing of the
mixed-precision ABI (tests/test_q32_refined_boundary.py holds that line; here: the C layer reaches host_q32/
and the new kernel weakly)."""
import ctypes
import os

import pytest

from test_device_api_emul import PRELUDE, needs_emul, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "iterative-solver_amd")
LIBDIR = os.path.join(PKG, "lib")
EMUL = os.path.join(ROOT, "oracle", "build")

SSP_NAMES = ["ssp_rows_export_quantised"]
C_NAMES = ["IterativeSolverHbmSetRefineAction", "IterativeSolverHbmRefineStatistics", "IterativeSolverHbmQStorage",
           "IterativeSolverHbmQuantise", "IterativeSolverHbmQuantiseDevice"]


def test_libraries_export_the_new_names():
    so = ctypes.CDLL(os.path.join(LIBDIR, "libsubspace_hip.so"), mode=ctypes.RTLD_GLOBAL)
    assert not [n for n in SSP_NAMES if not hasattr(so, n)]
    it = ctypes.CDLL(os.path.join(LIBDIR, "libitsolv_hbm.so"))
    assert not [n for n in C_NAMES if not hasattr(it, n)]
    # the C++ face between host/ and host_q32/ stays inside the library
    assert not hasattr(it, "make_rc_davidson_q32")


def test_bindings_declare_the_new_names_in_sets_of_their_own():
    import iterative_solver
    import subspace_hip as sh

    assert set(SSP_NAMES) <= set(sh.EXPORTS) and set(SSP_NAMES) == set(sh.OPTIONAL_ROWS_Q)
    assert not set(sh.OPTIONAL_ROWS_Q) & (set(sh.OPTIONAL) | set(sh.OPTIONAL_Q32) | set(sh.OPTIONAL_REFINED) |
                                          set(sh.OPTIONAL_ROWS))
    assert set(sh.OPTIONAL_ROWS) == {"ssp_rows_import", "ssp_rows_export"}
    assert len(sh.load_library().ssp_rows_export_quantised.argtypes) == 8
    assert sorted(iterative_solver.REFINE_SIG) == sorted(C_NAMES)
    assert not set(iterative_solver.REFINE_SIG) & set(iterative_solver.DEVICE_SIG)
    it = iterative_solver._load()
    assert len(it.IterativeSolverHbmSetRefineAction.argtypes) == 2
    assert len(it.IterativeSolverHbmRefineStatistics.argtypes) == 3
    assert len(it.IterativeSolverHbmQuantiseDevice.argtypes) == 3
    assert it.IterativeSolverHbmQStorage() == 0  # no instance
    assert it.IterativeSolverHbmRefineStatistics(None, None, None) == 1


def test_the_callback_typedef_is_no_exported_function():
    from test_boundary import declared_functions

    names = declared_functions("iterative_solver_c.h")
    assert "itsolv_refine_action_fn" not in names and set(C_NAMES) <= set(names)


@needs_emul
def test_the_c_layer_holds_no_strong_reference_to_the_new_entry_points():
    """libitsolv_emul.so is this tree's host/*.cpp without host_q32/, over a vector library without the export
    that rounds: it loads with immediate binding and exports the new calls."""
    ctypes.CDLL(os.path.join(EMUL, "libssp_emul.so"), mode=ctypes.RTLD_GLOBAL | os.RTLD_NOW)
    it = ctypes.CDLL(os.path.join(EMUL, "libitsolv_emul.so"), mode=os.RTLD_NOW)
    assert not [n for n in C_NAMES if not hasattr(it, n)]


LOAD_WITHOUT = PRELUDE + r"""
lib = sh.load_library()
assert not hasattr(lib, "ssp_rows_export_quantised")
with sh.Context(0) as ctx:
    rows = sh.DeviceRows(ctx, 2, 5)
    v = ctx.alloc(5)
    try:
        ctx.rows_export_quantised([v], rows)
    except sh.SspError as e:
        assert e.code == 7, e
    else:
        raise AssertionError("a call without the entry point did not raise")
    iterative_solver.use_context(ctx)
    s = iterative_solver.LinearEigensystem(5, 1, hermitian=True)
    assert s.q_storage == 8 and s.quantise(rows) == 0 and s.quantise(np.ones((1, 5))) == 0
    s.finalize()
print("ok")
"""


@needs_emul
def test_bindings_load_a_library_without_the_new_entry_points():
    r = run(LOAD_WITHOUT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_host_sources_name_the_f32_side_only_through_the_face():
    host = os.path.join(PKG, "host")
    text = open(os.path.join(host, "iterative_solver_c.cpp")).read()
    assert "hbm_handlers_f32.h" not in text and "hbm_vec_f32.h" not in text
    assert "__attribute__((weak))" in open(os.path.join(host, "rc_solver.h")).read()
    assert os.path.exists(os.path.join(PKG, "host_q32", "rc_q32.cpp"))
