"""The boundary of the mixed-precision layer (f32 storage, f64 arithmetic), checked without a GPU:
the libraries export the new C ABI, the Python bindings keep loading a library that lacks it (the CPU
emulation of the f64 ABI that the host tests run on), the solver templates compile for Q != R, and the
new reduction kernel's hand-off to the last workgroup is the write-through form in the emitted ISA."""
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
HIPCC = "/opt/rocm/bin/hipcc"

SSP_NAMES = ["ssp_alloc_f32", "ssp_free_f32", "ssp_upload_f32", "ssp_download_f32", "ssp_fill_f32", "ssp_scal_f32",
             "ssp_mx_copy", "ssp_mx_axpy", "ssp_mx_dot", "ssp_mx_gemm_inner", "ssp_mx_gemm_outer"]
ITSOLV_NAMES = ["itsolv_davidson_dense_q32", "itsolv_davidson_synth_q32"]


def test_libraries_export_the_mixed_precision_abi():
    so = ctypes.CDLL(os.path.join(LIBDIR, "libsubspace_hip.so"), mode=ctypes.RTLD_GLOBAL)
    assert not [n for n in SSP_NAMES if not hasattr(so, n)]
    it = ctypes.CDLL(os.path.join(LIBDIR, "libitsolv_hbm.so"))
    assert not [n for n in ITSOLV_NAMES if not hasattr(it, n)]


def test_bindings_list_and_declare_the_new_names():
    import itsolv_hbm as ih
    import subspace_hip as sh

    assert set(SSP_NAMES) <= set(sh.EXPORTS) and set(SSP_NAMES) == set(sh.OPTIONAL)
    assert set(ITSOLV_NAMES) <= set(ih.EXPORTS) and set(ITSOLV_NAMES) == set(ih.OPTIONAL)
    lib = sh.load_library()
    assert lib.ssp_mx_gemm_outer.argtypes is not None and len(lib.ssp_mx_gemm_outer.argtypes) == 11
    assert len(ih.load_library().itsolv_davidson_dense_q32.argtypes) == 6
    assert sh.DeviceVector(None, 3, 0).dtype == "float64"
    assert sh.DeviceVector(None, 3, 0, dtype="float32").dtype == "float32"
    with pytest.raises(TypeError):
        sh.DeviceVector(None, 3, 0, dtype="float16")


EMUL_SCRIPT = r"""
import os, sys
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "iterative-solver_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import itsolv_hbm as ih
import subspace_hip as sh
EMUL = os.path.join(ROOT, "oracle", "build")
sh.LIB_PATH = os.path.join(EMUL, "libssp_emul.so")
ih.LIB_PATH = os.path.join(EMUL, "libitsolv_emul.so")
lib = sh.load_library()
assert not hasattr(lib, "ssp_mx_copy"), "the emulation is not expected to have the mixed entry points"
ih.load_library()
with sh.Context(0) as ctx:
    x = ctx.upload(np.arange(5.0))
    y = ctx.upload(np.ones(5))
    assert ctx.dot(x, y) == 10.0  # the f64 surface works as before
    calls = [lambda: ctx.mx_copy(x, y), lambda: ctx.mx_axpy(1.0, x, y), lambda: ctx.mx_dot(x, y),
             lambda: ctx.mx_gemm_inner([x], [y]), lambda: ctx.mx_gemm_outer(np.ones((1, 1)), [x], [y]),
             lambda: ctx.alloc(5, np.float32), lambda: ctx.upload(np.ones(5), np.float32),
             lambda: ih.davidson_dense(ctx, np.eye(4), q32=True, nroots=1),
             lambda: ih.davidson_synthetic(ctx, 64, 0.1, 1, 1, q32=True)]
    for i, f in enumerate(calls):
        try:
            f()
        except sh.SspError as e:
            assert e.code == 7, (i, e)
        else:
            raise AssertionError(f"call {i} did not raise")
    r = ih.davidson_dense(ctx, np.diag(np.arange(1.0, 9.0)), nroots=1, convergence_threshold=1e-8)
    assert r["converged"] and abs(r["eigenvalues"][0] - 1.0) < 1e-8
print("ok")
"""


@pytest.mark.skipif(not os.path.exists(os.path.join(EMUL, "libssp_emul.so")), reason="needs `make -C oracle`")
def test_bindings_load_a_library_without_the_mixed_entry_points():
    """The CPU emulation (oracle/) implements the f64 ABI only: the bindings must load it, and a mixed
    call must raise SSP_ERR_UNSUPPORTED instead of an AttributeError at load time."""
    r = subprocess.run([sys.executable, "-c", EMUL_SCRIPT, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


TU = r"""
#include "itsolv_hbm/hbm_handlers_f32.h"
#include "itsolv_hbm/solvers.h"
using namespace molpro::linalg;
template class itsolv::LinearEigensystemDavidson<hbm::Vec, hbm::VecF32, hbm::SparseP>;
template class hbm::ArrayHandlerMx<hbm::Vec, hbm::VecF32>;
template class hbm::ArrayHandlerMx<hbm::VecF32, hbm::Vec>;
template class hbm::ArrayHandlerMx<hbm::VecF32, hbm::VecF32>;
static_assert(std::is_same_v<hbm::VecF32::value_type, double>, "the logical element type stays double");
static_assert(std::is_same_v<hbm::VecF32::storage_type, float>, "the storage is binary32");
auto solver() {
  return std::make_unique<itsolv::LinearEigensystemDavidson<hbm::Vec, hbm::VecF32, hbm::SparseP>>(hbm::make_handlers_q32());
}
"""


def makefile_cxxflags():
    out = subprocess.run(["make", "-pn", "-C", PKG, "clean"], capture_output=True, text=True, timeout=120).stdout
    for line in out.splitlines():
        if line.startswith("CXXFLAGS := ") or line.startswith("CXXFLAGS = "):
            return line.split("=", 1)[1].split()
    raise AssertionError("CXXFLAGS not found in the Makefile's database")


def test_davidson_compiles_with_an_f32_q_space():
    flags = makefile_cxxflags()
    assert "-std=c++17" in flags
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "q32_tu.cpp")
        with open(src, "w") as f:
            f.write(TU)
        r = subprocess.run([os.environ.get("CXX", "g++")] + flags + ["-fsyntax-only", src], cwd=PKG, capture_output=True,
                           text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]


def test_f64_headers_do_not_see_the_f32_ones():
    inc = os.path.join(PKG, "include", "itsolv_hbm")
    for name in os.listdir(inc):
        if name in ("hbm_vec_f32.h", "hbm_handlers_f32.h"):
            continue
        text = open(os.path.join(inc, name)).read()
        assert "hbm_vec_f32.h" not in text and "hbm_handlers_f32.h" not in text, name
    for name in os.listdir(os.path.join(PKG, "host")):  # host/ is also built against the f64 emulation
        text = open(os.path.join(PKG, "host", name)).read()
        assert "ssp_mx_" not in text and "_f32" not in text, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mixed_dot_hands_its_partials_off_write_through():
    """k_mx_dot carries ssp::fold_tail: the checks of tests/test_fold_tail_isa.py on its gfx950 assembly."""
    from test_fold_tail_isa import fold_tail_violations, kernels

    csrc = os.path.join(PKG, "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernels_mixed.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "kernels_mixed.hip"), "-o", out],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        found = [(name, fold_tail_violations(ins)) for name, ins in kernels(open(out).read()) if "k_mx_dot" in name]
    assert len(found) == 3, [n for n, _ in found]
    for name, bad in found:
        assert bad == [], (name, bad)
