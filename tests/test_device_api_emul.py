"""The device forms of the reverse-communication API (include/iterative_solver_c.h, IterativeSolverHbm*Device)
on the CPU, over the emulation of the f64 C ABI: there "device" memory is host memory and the vector library
has no ssp_rows_*, so the C layer's weakly bound fallback runs (one ssp_copy per 16-byte aligned row, one
ssp_scal_copy where a scale is pending) -- which is what makes the whole C-layer logic testable without a GPU.
The comparison is tests/device_api_cases.py's: the host route and the device route, call by call, bit for bit.
The same over the HIP library: tests/test_device_api_gpu.py."""
import ctypes
import os
import subprocess
import sys

import pytest

from test_distributed import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "iterative-solver_amd")
LIBDIR = os.path.join(PKG, "lib")
EMUL = os.path.join(ROOT, "oracle", "build")
needs_emul = pytest.mark.skipif(not os.path.exists(os.path.join(EMUL, "libitsolv_emul.so")), reason="needs `make -C oracle`")

SSP_NAMES = ["ssp_rows_import", "ssp_rows_export"]
C_NAMES = ["IterativeSolverHbmAddVectorDevice", "IterativeSolverHbmSolutionDevice", "IterativeSolverHbmAddValueDevice",
           "IterativeSolverHbmEndIterationDevice", "IterativeSolverHbmSetDiagonalsDevice",
           "IterativeSolverHbmDiagonalsDevice"]

PRELUDE = r"""
import os, sys
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "iterative-solver_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import iterative_solver
import itsolv_hbm as ih
import subspace_hip as sh
EMUL = os.path.join(ROOT, "oracle", "build")
sh.LIB_PATH = os.path.join(EMUL, "libssp_emul.so")
ih.LIB_PATH = os.path.join(EMUL, "libitsolv_emul.so")
iterative_solver.LIB_PATH = os.path.join(EMUL, "libitsolv_emul.so")
import device_api_cases as dc
import rc_problems as rp
assert not hasattr(sh.load_library(), "ssp_rows_import"), "the emulation is not expected to have the row-block entry points"
"""

SINGLE = PRELUDE + r"""
from test_python_api_gpu import hamiltonian
ctx = sh.Context(0)
iterative_solver.use_context(ctx)
assert all(hasattr(iterative_solver._load(), n) for n in iterative_solver.DEVICE_SIG)
calls = 0
# LinearEigensystem on the dense fixtures, without and with a P space (AddP through host arrays, then device calls)
for name, nroot, np_ in (("bh", 2, 0), ("hf", 3, 0), ("bh", 3, 4), ("hf", 1, 0)):
    h = hamiltonian(name, 1e-8)
    n = h.shape[0]
    make = dc.eigen_solver(n, nroot, options=f"MAX_SIZE_QSPACE={6 * nroot},RESET_D=8")
    hl, dl, hr, dr = dc.both_routes(make, lambda s: rp.loop_eigen(s, h, nroot, np_), ctx)
    dc.assert_same_log(hl, dl)
    assert hr == dr and len(hl) > 4 and (np_ == 0 or hl[0][0] == "add_p"), (name, hr, dr)
    calls += len(hl)
    # the loop with the solution call at the end, to convergence
    d = np.diag(h).copy()
    guess = sorted(np.argsort(d, kind="stable")[:nroot])
    hl, dl, hr, dr = dc.both_routes(make, lambda s: dc.loop_davidson(s, nroot, n, lambda x: x @ h, d, guess), ctx)
    dc.assert_same_log(hl, dl)
    assert hl[-1][0] == "solution" and np.all(hl[-1][2] < 1e-7), hl[-1][2]
# LinearEquations
h = hamiltonian("bh", 1e-8) + 3.0 * np.eye(28)
rhs = np.vstack([h[:, 0] + 1.0, np.arange(1.0, 29.0)])
make = lambda: iterative_solver.LinearEquations(rhs, thresh=1e-9, hermitian=True)
hl, dl, hr, dr = dc.both_routes(make, lambda s: dc.loop_davidson(s, 2, 28, lambda x: x @ h, np.diag(h).copy(), [0, 1]), ctx)
dc.assert_same_log(hl, dl)
assert np.all(hl[-1][2] < 1e-7) and np.allclose(hr[0] @ h, rhs, atol=1e-6), hl[-1][2]
# NonLinearEquations (DIIS) and Optimize (BFGS, through AddValueDevice) on the quadratic form
hq = rp.quadratic_matrix(20, 10.0)
for optimize in (False, True):
    make = (lambda: iterative_solver.Optimize(20, thresh=1e-8)) if optimize else \
        (lambda: iterative_solver.NonLinearEquations(20, thresh=1e-8))
    hl, dl, hr, dr = dc.both_routes(make, lambda s: rp.loop_quadratic(s, hq, optimize), ctx)
    dc.assert_same_log(hl, dl)
    assert hr[1] == dr[1] and hr[1] > 3 and np.allclose(hr[0][-1][2], 1.0, atol=1e-6), hr[1]
    assert {e[0] for e in hl} == ({"add_value", "end_iteration"} if optimize else {"add_vector", "end_iteration"})
# diagonals round trip through device memory
s = iterative_solver.LinearEigensystem(28, 2)
d = ctx.upload(np.arange(28.0) ** 2 - 0.5)
out = ctx.alloc(28)
iterative_solver._dcall("IterativeSolverHbmSetDiagonalsDevice", d.ptr)
iterative_solver._dcall("IterativeSolverHbmDiagonalsDevice", out.ptr)
host = np.zeros(28)
iterative_solver._call("IterativeSolverDiagonals", host.ctypes.data_as(iterative_solver.PD))
assert np.array_equal(out.numpy(), np.arange(28.0) ** 2 - 0.5) and np.array_equal(host, out.numpy())
# a numpy array beside a device array is a TypeError; so is nothing else
rows = sh.DeviceRows(ctx, 2, 28)
for f in (lambda: s.add_vector(np.zeros((2, 28)), rows), lambda: s.end_iteration(rows, np.zeros((2, 28))),
          lambda: s.add_value(0.0, rows.row(0), np.zeros(28)), lambda: s.solution([0], np.zeros(28), rows.row(0))):
    try:
        f()
    except TypeError:
        pass
    else:
        raise AssertionError("mixed host and device arrays did not raise TypeError")
try:
    s.add_vector(sh.DeviceRows(ctx, 2, 27), sh.DeviceRows(ctx, 2, 27))
except ValueError as e:
    assert "range" in str(e)
else:
    raise AssertionError("rows of the wrong length did not raise")
s.finalize()
print("calls compared:", calls)
print("ok")
"""

MISALIGNED = PRELUDE + r"""
from test_python_api_gpu import hamiltonian
ctx = sh.Context(0)
iterative_solver.use_context(ctx)
h = hamiltonian("bh", 1e-8)
n, nroot = 28, 2
d = np.diag(h).copy()
guess = sorted(np.argsort(d, kind="stable")[:nroot])
ref_log = []
s = dc.eigen_solver(n, nroot)()
dc.loop_davidson(dc.Recorded(s, s, ref_log), nroot, n, lambda x: x @ h, d, guess)
s.finalize()
# the same loop through the device calls, after a refused call on the same instance
s = dc.eigen_solver(n, nroot)()
buf = ctx.upload(np.zeros(2 * (2 * n + 2)))
assert buf.ptr % 16 == 0
x0 = np.zeros((nroot, n))
for k, i in enumerate(guess):
    x0[k, i] = 1.0
for ld, base in ((n, 1), (n + 1, 0)):  # every row, or every other row, at 8 mod 16
    px = sh.DeviceRows(ctx, nroot, n, ld, ptr=buf.ptr + 8 * base)
    pg = sh.DeviceRows(ctx, nroot, n, ld, ptr=buf.ptr + 8 * (base + nroot * ld + (nroot * ld + base) % 2))
    px.upload(x0)
    pg.upload(x0 @ h)
    for call in (lambda: s.add_vector(px, pg), lambda: s.end_iteration(px, pg), lambda: s.solution([0, 1], px, pg)):
        try:
            call()
        except RuntimeError as e:
            assert "UNSUPPORTED" in str(e) and "16-byte aligned" in str(e), e
        else:
            raise AssertionError("a misaligned row over the emulation did not raise")
    assert np.array_equal(px.numpy(), x0) and np.array_equal(pg.numpy(), x0 @ h)  # nothing was staged or written
assert s.statistics() == {"iterations": 0, "r_creations": 0, "q_creations": 0}, s.statistics()
log = []
dc.loop_davidson(dc.Recorded(dc.ViaDevice(s, ctx), s, log), nroot, n, lambda x: x @ h, d, guess)
dc.assert_same_log(ref_log, log)
s.finalize()
print("ok")
"""

SHARDED = PRELUDE + r"""
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
comm = sh.HubComm(rank, world, "127.0.0.1", int(os.environ["SSP_HUB_PORT"]))
ctx = sh.Context(0)
ctx.attach_host_comm(comm)
iterative_solver.use_context(ctx)
n, nroot = 61, 3
m = np.ones((n, n)) + np.diag(3.0 * np.arange(1, n + 1))
make = dc.eigen_solver(n, nroot)
loop = lambda s: dc.loop_davidson(s, nroot, n, lambda x: x @ m, np.diag(m).copy(), [0, 1, 2])
hl, dl, hr, dr = dc.both_routes(make, loop, ctx, comm=comm)
dc.assert_same_log(hl, dl)
s = make()
assert (s.offset, s.local) == sh.shard_range(n, world, rank)
s.finalize()
assert hl[-1][0] == "solution" and np.all(hl[-1][2] < 1e-7) and len(hl) > 6
comm.barrier()
print("ok")
"""


SOLVE = PRELUDE + r"""
import ctypes
from test_python_api import RayleighQuotient
ctx = sh.Context(0)
iterative_solver.use_context(ctx)


def view(v):  # over the emulation device memory is host memory
    return np.ctypeslib.as_array((ctypes.c_double * v.n).from_address(v.ptr))


class OnDevice(iterative_solver.Problem):
    # the reference's Python test problem on device arrays; the preconditioner is Problem's default
    def __init__(self, p):
        super().__init__()
        self.p = p

    def residual(self, x, g):
        return self.p.residual(view(x), view(g))

    def action(self, x, g):
        for k in range(x.m):
            self.p.action(view(x.row(k)).reshape(1, -1), view(g.row(k)).reshape(1, -1))

    def diagonals(self, d):
        return self.p.diagonals(view(d))


class NonLinearOnDevice(OnDevice):
    def precondition(self, residual, shift=None, diagonals=None):
        assert residual.m == 1 and isinstance(diagonals, sh.DeviceVector)
        self.p.precondition(view(residual.row(0)), float(shift[0]), view(diagonals))


# LinearEigensystem: default initial guess (select + sparse copy) and default preconditioner (Context.precondition)
prob = RayleighQuotient(8, 0.1)
s = iterative_solver.LinearEigensystem(8, 2)
x, g = sh.DeviceRows(ctx, 2, 8), sh.DeviceRows(ctx, 2, 8)
s.solve(x, g, OnDevice(prob), generate_initial_guess=True)
s.solution([0, 1], x, g)
assert np.all(s.errors < 1e-7), s.errors
assert np.allclose(s.eigenvalues, prob.eigenvalues[:2], atol=1e-7)
assert np.allclose(np.abs(x.numpy() @ prob.eigenvectors[:, :2]), np.eye(2) * np.linalg.norm(x.numpy(), axis=1), atol=1e-6)
s.finalize()
# NonLinearEquations: one DeviceVector each
prob = RayleighQuotient(4, 0.01)
xv, gv = ctx.upload(np.array([1.0, 0.0, 0.0, 0.0])), ctx.alloc(4)
s = iterative_solver.NonLinearEquations(4)
s.solve(xv, gv, NonLinearOnDevice(prob))
s.solution([0], xv, gv)
sol = xv.numpy()
sol = sol * prob.eigenvectors[0, 0] / sol[0]
assert abs(prob.residual(sol, np.zeros(4)) - prob.eigenvalues[0]) < 1e-7
s.finalize()
print("ok")
"""


@needs_emul
def test_python_solve_runs_on_device_arrays():
    r = run(SOLVE)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def run(script, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", script, ROOT], capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


@needs_emul
def test_host_and_device_routes_agree_bit_for_bit_through_the_fallback():
    r = run(SINGLE)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


@needs_emul
def test_a_misaligned_row_over_the_emulation_is_unsupported_and_leaves_the_instance_usable():
    r = run(MISALIGNED)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


@needs_emul
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_device_rows_hold_each_ranks_range(world):
    port = free_port()
    procs = [subprocess.Popen([sys.executable, "-c", SHARDED, ROOT],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), SSP_HUB_PORT=str(port),
                                       OMP_NUM_THREADS="1"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]


# ---- boundary -------------------------------------------------------------------------------------
def test_libraries_export_the_device_forms():
    so = ctypes.CDLL(os.path.join(LIBDIR, "libsubspace_hip.so"), mode=ctypes.RTLD_GLOBAL)
    assert not [n for n in SSP_NAMES if not hasattr(so, n)]
    it = ctypes.CDLL(os.path.join(LIBDIR, "libitsolv_hbm.so"))
    assert not [n for n in C_NAMES if not hasattr(it, n)]


def test_bindings_list_the_new_names_in_a_set_of_their_own():
    import iterative_solver
    import subspace_hip as sh

    assert set(SSP_NAMES) <= set(sh.EXPORTS) and set(SSP_NAMES) == set(sh.OPTIONAL_ROWS)
    assert not set(sh.OPTIONAL_ROWS) & (set(sh.OPTIONAL) | set(sh.OPTIONAL_Q32) | set(sh.OPTIONAL_REFINED))
    lib = sh.load_library()
    assert len(lib.ssp_rows_import.argtypes) == 6 and len(lib.ssp_rows_export.argtypes) == 7
    assert sorted(iterative_solver.DEVICE_SIG) == sorted(C_NAMES)
    it = iterative_solver._load()
    assert len(it.IterativeSolverHbmAddVectorDevice.argtypes) == 4
    assert len(it.IterativeSolverHbmAddValueDevice.argtypes) == 3
    assert len(it.IterativeSolverHbmSolutionDevice.argtypes) == 5


@needs_emul
def test_the_c_layer_holds_no_strong_reference_to_the_row_entry_points():
    """libitsolv_emul.so is this tree's host/*.cpp over a vector library without ssp_rows_*: it loads with
    immediate binding (as Python loads it) and exports the device forms."""
    ctypes.CDLL(os.path.join(EMUL, "libssp_emul.so"), mode=ctypes.RTLD_GLOBAL | os.RTLD_NOW)
    it = ctypes.CDLL(os.path.join(EMUL, "libitsolv_emul.so"), mode=os.RTLD_NOW)
    assert not [n for n in C_NAMES if not hasattr(it, n)]


LOAD_WITHOUT = PRELUDE + r"""
lib = sh.load_library()
with sh.Context(0) as ctx:
    rows = sh.DeviceRows(ctx, 2, 5)
    rows.upload(np.arange(10.0).reshape(2, 5))
    assert np.array_equal(rows.numpy(), np.arange(10.0).reshape(2, 5)) and rows.ld == 6
    v = ctx.alloc(5)
    for f in (lambda: ctx.rows_import(rows, [v]), lambda: ctx.rows_export([v], rows)):
        try:
            f()
        except sh.SspError as e:
            assert e.code == 7, e
        else:
            raise AssertionError("a call without the entry point did not raise")
print("ok")
"""


@needs_emul
def test_bindings_load_a_library_without_the_row_entry_points():
    r = run(LOAD_WITHOUT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
