"""iterative_solver on MI355X: the reference's Python API (python/iterative_solver, a Cython
extension over src/molpro/linalg/IterativeSolverC.h) as a ctypes binding of the same C API in
libitsolv_hbm.so (include/iterative_solver_c.h).  Class names, constructor arguments and methods
follow the reference (iterative_solver_extension.pyx); the Q space and all subspace operations
live in HBM, the parameter/residual arrays the caller passes stay numpy arrays -- or, for a caller whose
action runs on the GPU, subspace_hip.DeviceRows (device memory: the IterativeSolverHbm*Device calls).

Available: LinearEigensystem and LinearEquations (Davidson), NonLinearEquations (DIIS), Optimize
(BFGS, SD).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from .problem import Problem

__all__ = ["Problem", "IterativeSolver", "LinearEigensystem", "NonLinearEquations", "LinearEquations", "Optimize"]

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_HERE, "lib", "libitsolv_hbm.so")
_lib = None

P, D, Z, I = C.c_void_p, C.c_double, C.c_size_t, C.c_int
PD, PZ, PI = C.POINTER(C.c_double), C.POINTER(C.c_size_t), C.POINTER(C.c_int)
APPLY_P = C.CFUNCTYPE(None, PD, PD, C.c_size_t, PZ)
# The device forms of the calls that stage R (include/iterative_solver_c.h): device addresses, this
# rank's shard, row k at p + k * ld.
DEVICE_SIG = {
    "IterativeSolverHbmAddVectorDevice": (Z, [Z, P, P, Z]),
    "IterativeSolverHbmSolutionDevice": (None, [I, PI, P, P, Z]),
    "IterativeSolverHbmAddValueDevice": (Z, [D, P, P]),
    "IterativeSolverHbmEndIterationDevice": (Z, [Z, P, P, Z]),
    "IterativeSolverHbmSetDiagonalsDevice": (None, [P]),
    "IterativeSolverHbmDiagonalsDevice": (None, [P]),
}
# The Q space in f32 and the refined residuals (Q_STORAGE / Q_REFINE options of LinearEigensystem): declared
# only when the loaded library has them, and a set of their own (DEVICE_SIG stays the device forms).
REFINE_ACTION = C.CFUNCTYPE(None, Z, P, P, Z, P)
REFINE_SIG = {
    "IterativeSolverHbmSetRefineAction": (I, [REFINE_ACTION, P]),
    "IterativeSolverHbmRefineStatistics": (I, [PI, PI, PD]),
    "IterativeSolverHbmQStorage": (Z, []),
    "IterativeSolverHbmQuantise": (Z, [Z, PD]),
    "IterativeSolverHbmQuantiseDevice": (Z, [Z, P, Z]),
}
# The refined mode under a Q-space limit (option Q_REFINE_DSPACE): declared in the same way, a set of its own.
DSPACE_SIG = {
    "IterativeSolverHbmRefineDspaceStats": (I, [PI, PI]),
}
_ctx = None  # the context given to use_context


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} missing: run `make -C iterative-solver_amd`")
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        sig = {
            "IterativeSolverLinearEigensystemInitialize": (None, [Z, Z, PZ, PZ, D, D, I, I, C.c_char_p, C.c_int64,
                                                                  C.c_char_p, C.c_char_p]),
            "IterativeSolverLinearEquationsInitialize": (None, [Z, Z, PZ, PZ, PD, D, D, D, I, I, C.c_char_p, C.c_int64,
                                                                C.c_char_p, C.c_char_p]),
            "IterativeSolverNonLinearEquationsInitialize": (None, [Z, PZ, PZ, D, I, C.c_char_p, C.c_int64, C.c_char_p,
                                                                   C.c_char_p]),
            "IterativeSolverOptimizeInitialize": (None, [Z, PZ, PZ, D, D, I, I, C.c_char_p, C.c_int64, C.c_char_p,
                                                         C.c_char_p]),
            "IterativeSolverFinalize": (None, []),
            "IterativeSolverAddVector": (Z, [Z, PD, PD, I]),
            "IterativeSolverSolution": (None, [I, PI, PD, PD, I]),
            "IterativeSolverAddValue": (Z, [D, PD, PD, I]),
            "IterativeSolverEndIteration": (Z, [Z, PD, PD, I]),
            "IterativeSolverEndIterationNeeded": (I, []),
            "IterativeSolverAddP": (Z, [Z, Z, PZ, PZ, PD, PD, PD, PD, I, APPLY_P]),
            "IterativeSolverErrors": (None, [PD]),
            "IterativeSolverEigenvalues": (None, [PD]),
            "IterativeSolverWorkingSetEigenvalues": (None, [PD]),
            "IterativeSolverSuggestP": (Z, [PD, PD, Z, D, PZ]),
            "IterativeSolverPrintStatistics": (None, []),
            "IterativeSolverNonLinear": (I, []),
            "IterativeSolverHasValues": (I, []),
            "IterativeSolverHasEigenvalues": (I, []),
            "IterativeSolverSetDiagonals": (None, [PD]),
            "IterativeSolverDiagonals": (None, [PD]),
            "IterativeSolverValue": (D, []),
            "IterativeSolverVerbosity": (I, []),
            "IterativeSolverMaxIter": (I, []),
            "IterativeSolverSetMaxIter": (None, [I]),
            "IterativeSolver_mpicomm_global": (C.c_int64, []),
            "IterativeSolverHbmSetContext": (I, [P]),
            "IterativeSolverHbmSetThrow": (I, [I]),
            "IterativeSolverHbmStatistics": (I, [PI, PI, PI]),
            "IterativeSolverHbmLastError": (C.c_char_p, []),
            "IterativeSolverHbmInstanceId": (C.c_uint64, []),
            "IterativeSolverHbmFinalizeInstance": (I, [C.c_uint64]),
            "IterativeSolverHbmMpiActive": (I, []),
            "IterativeSolverHbmMpiAttach": (I, [P, C.c_int64, C.c_char_p]),
        }
        for name, (res, args) in sig.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        for name, (res, args) in {**DEVICE_SIG, **REFINE_SIG, **DSPACE_SIG}.items():  # declared only when the library has them
            f = getattr(lib, name, None)
            if f is not None:
                f.restype, f.argtypes = res, args
        lib.IterativeSolverHbmSetThrow(0)  # ctypes cannot unwind C++ exceptions: record them instead
        _lib = lib
    return _lib


def _call(name, *args):
    lib = _load()
    # The flag is the process's, not this binding's: another user of the library in the same process (a
    # Fortran or C++ caller) may have restored throwing, and an exception cannot unwind through ctypes.
    lib.IterativeSolverHbmSetThrow(0)
    r = getattr(lib, name)(*args)
    err = lib.IterativeSolverHbmLastError()
    if err:
        raise RuntimeError(err.decode())
    return r


def _d(a):
    return a.ctypes.data_as(PD)


def use_context(ctx):
    """Run the instances created after this call on `ctx` (a subspace_hip.Context, possibly with a
    communicator attached); None restores the default single-rank context on device 0."""
    global _ctx
    _call("IterativeSolverHbmSetContext", ctx.handle if ctx is not None else None)
    _ctx = ctx


def _dcall(name, *args):
    if not hasattr(_load(), name):
        raise RuntimeError(f"{name}: the loaded library has no device forms of the reverse-communication calls")
    return _call(name, *args)


def _rcall(name, *args):
    if not hasattr(_load(), name):
        raise RuntimeError(f"{name}: the loaded library has no refined mode of the reverse-communication calls")
    return _call(name, *args)


def _option(options, key):
    """The value of `key` in a "k1=v1,k2=v2" options string (keys case-insensitive), or None."""
    for field in options.replace(";", ",").split(","):
        k, sep, v = field.replace(":", "=", 1).partition("=")
        if sep and k.strip().upper() == key:
            return v.strip()
    return None


def _is_device(a):
    sh = sys.modules.get("subspace_hip")  # device arrays can only come from that module
    return sh is not None and isinstance(a, (sh.DeviceRows, sh.DeviceVector))


def _device_pair(solver, first, second):
    """None for two numpy arrays; (rows, address, address, ld) for two device arrays of one shape
    (subspace_hip.DeviceRows, or a DeviceVector where one row is meant).  A numpy array beside a device
    array is a TypeError."""
    if not _is_device(first) and not _is_device(second):
        return None
    if not (_is_device(first) and _is_device(second)):
        raise TypeError("parameters and action/residual are both numpy arrays or both device arrays")
    shapes = [(getattr(a, "m", 1), a.n, getattr(a, "ld", a.n)) for a in (first, second)]
    if shapes[0] != shapes[1]:
        raise ValueError(f"device arrays of different shapes (rows, length, ld): {shapes[0]} and {shapes[1]}")
    if any(getattr(a, "dtype", np.float64) != np.float64 for a in (first, second)):
        raise TypeError("device arrays are float64")
    if shapes[0][1] != solver.local:
        raise ValueError(f"device rows hold this rank's range of {solver.local} elements, not {shapes[0][1]}")
    return shapes[0][0], first.ptr, second.ptr, shapes[0][2]


def statistics():
    it, r, q = C.c_int(), C.c_int(), C.c_int()
    if _load().IterativeSolverHbmStatistics(C.byref(it), C.byref(r), C.byref(q)) != 0:
        raise RuntimeError("no active solver")
    return {"iterations": it.value, "r_creations": r.value, "q_creations": q.value}


def _flat(a):
    if not (a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]):
        raise ValueError("parameter/residual arrays must be C-contiguous float64")
    return a


class IterativeSolver:
    """Base of LinearEigensystem / NonLinearEquations (reference iterative_solver_extension.pyx)."""

    def __init__(self, n, nroot=1):
        self.n = n
        self.nroot = nroot
        self.value = None
        self._id = 0
        self.offset, self.local = 0, n  # this rank's range, set by _register_range

    def _register_range(self, rb, re):
        self.offset, self.local = rb.value, re.value - rb.value

    def _register(self):
        """Called after the C layer pushed this object's instance: remember its id."""
        self._id = int(_load().IterativeSolverHbmInstanceId())
        self._active = self._id != 0

    def _check_top(self):
        # The C layer drives its top instance only (reference IterativeSolverCMPI.cpp); a call
        # through an older object while a newer one is alive would silently drive the newer one.
        if not getattr(self, "_active", False):
            raise RuntimeError("this solver has been finalized")
        if int(_load().IterativeSolverHbmInstanceId()) != self._id:
            raise RuntimeError("another IterativeSolver instance is active (created later and not finalized)")

    def __del__(self):
        # Removes this object's own instance wherever it is in the C layer's stack, never another's.
        try:
            if getattr(self, "_active", False):
                _load().IterativeSolverHbmFinalizeInstance(self._id)
                self._active = False
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def mpicomm_compute(self):
        """The communicator the instances use by default, as in the reference
        (iterative_solver_extension.pyx:27-31): IterativeSolver_mpicomm_global(), the Fortran handle of
        MPI_COMM_WORLD when the process has initialised MPI (the C layer then shards the vectors over its
        ranks), else 0 (no communicator: one rank, or the context set by use_context)."""
        return _mpicomm_compute()

    def finalize(self):
        if getattr(self, "_active", False):
            _load().IterativeSolverHbmFinalizeInstance(self._id)
            self._active = False

    def solution(self, roots, parameters, residual, sync=True):
        self._check_top()
        roots_ = (C.c_int * max(1, len(roots)))(*roots)
        dev = _device_pair(self, parameters, residual)
        if dev is not None:
            if dev[0] < len(roots):
                raise ValueError("solution: fewer device rows than roots")
            _dcall("IterativeSolverHbmSolutionDevice", len(roots), roots_, dev[1], dev[2], dev[3])
            return self.value
        _call("IterativeSolverSolution", len(roots), roots_, _d(_flat(parameters)), _d(_flat(residual)), int(sync))
        return self.value

    def add_vector(self, parameters, action, sync=True):
        self._check_top()
        dev = _device_pair(self, parameters, action)
        self._refine_ctx = parameters.ctx if dev is not None else None  # where a refine action's arrays live
        if dev is not None:
            r = int(_dcall("IterativeSolverHbmAddVectorDevice", *dev))
        else:
            nbuffer = parameters.shape[0] if parameters.ndim > 1 else 1
            r = int(_call("IterativeSolverAddVector", nbuffer, _d(_flat(parameters)), _d(_flat(action)), int(sync)))
        self._reraise_refine()
        return r

    # -- the Q space in f32 and refined residuals (options Q_STORAGE=f32, Q_REFINE=1 of LinearEigensystem) ----
    def set_refine_action(self, fn):
        """The action the refined mode forms its residuals with: fn(parameters, action) sets action[k] =
        H parameters[k].  Called from inside add_vector / add_p with numpy views of shape (m, n) of that call's
        own arrays, or, for a call on device arrays, with DeviceRows of m rows and the call's ld.  None clears."""
        self._check_top()
        if fn is None:
            _rcall("IterativeSolverHbmSetRefineAction", REFINE_ACTION(), None)
            self._refine_tramp = None
            return

        def tramp(nvec, p, g, ld, user):
            try:
                ctx = getattr(self, "_refine_ctx", None)
                if ctx is not None:
                    from subspace_hip import DeviceRows

                    fn(DeviceRows(ctx, nvec, self.local, ld, ptr=p), DeviceRows(ctx, nvec, self.local, ld, ptr=g))
                else:
                    x = np.ctypeslib.as_array((C.c_double * (nvec * ld)).from_address(p)).reshape(nvec, ld)
                    a = np.ctypeslib.as_array((C.c_double * (nvec * ld)).from_address(g)).reshape(nvec, ld)
                    fn(x, a)
            except BaseException as e:  # noqa: BLE001 - cannot unwind through the C layer: raised by the caller
                self._refine_exc = e

        tr = REFINE_ACTION(tramp)
        _rcall("IterativeSolverHbmSetRefineAction", tr, None)
        self._refine_tramp = tr  # keep alive for the solver's lifetime

    def _reraise_refine(self):
        e, self._refine_exc = getattr(self, "_refine_exc", None), None
        if e is not None:
            raise e

    def quantise(self, parameters):
        """Rounds parameter rows in place to the instance's Q storage format (nothing with Q_STORAGE=f64): what an
        initial guess that is not a unit vector needs before its action is formed in refined mode.  Returns
        the number of rows rounded."""
        self._check_top()
        if _is_device(parameters):
            if parameters.n != self.local:
                raise ValueError(f"device rows hold this rank's range of {self.local} elements, not {parameters.n}")
            return int(_rcall("IterativeSolverHbmQuantiseDevice", getattr(parameters, "m", 1), parameters.ptr,
                              getattr(parameters, "ld", parameters.n)))
        nbuffer = parameters.shape[0] if parameters.ndim > 1 else 1
        return int(_rcall("IterativeSolverHbmQuantise", nbuffer, _d(_flat(parameters))))

    @property
    def q_storage(self):
        """Bytes per stored Q element: 8, or 4 with Q_STORAGE=f32."""
        self._check_top()
        return int(_rcall("IterativeSolverHbmQStorage"))

    def refine_statistics(self):
        self._check_top()
        n, first, delta = C.c_int(), C.c_int(), C.c_double()
        if _rcall("IterativeSolverHbmRefineStatistics", C.byref(n), C.byref(first), C.byref(delta)) != 0:
            raise RuntimeError("no active solver")
        return {"refined_actions": n.value, "first_refined_iteration": first.value, "max_delta": delta.value}

    @property
    def refine_dspace_statistics(self):
        """With Q_REFINE_DSPACE=1: the D space's rebuilds and the actions spent on them (not among
        refine_statistics' refined_actions)."""
        self._check_top()
        r, a = C.c_int(), C.c_int()
        if _rcall("IterativeSolverHbmRefineDspaceStats", C.byref(r), C.byref(a)) != 0:
            raise RuntimeError("no active solver")
        return {"dspace_rebuilds": r.value, "dspace_actions": a.value}

    def add_value(self, value, parameters, action, sync=True):
        self._check_top()
        dev = _device_pair(self, parameters, action)
        if dev is not None:  # one row: the first of each array
            r = int(_dcall("IterativeSolverHbmAddValueDevice", value, dev[1], dev[2]))
        else:
            r = int(_call("IterativeSolverAddValue", value, _d(_flat(parameters)), _d(_flat(action)), int(sync)))
        self.value = value
        return r

    def end_iteration(self, parameters, residual, sync=True):
        self._check_top()
        dev = _device_pair(self, parameters, residual)
        # Q_REFINE_DSPACE=1: a D-space rebuild calls the refine action from inside, on this call's arrays
        self._refine_ctx = parameters.ctx if dev is not None else None
        try:
            return self._end_iteration(dev, parameters, residual, sync)
        finally:
            self._reraise_refine()

    def _end_iteration(self, dev, parameters, residual, sync):
        if dev is not None:
            return int(_dcall("IterativeSolverHbmEndIterationDevice", *dev))
        nbuffer = parameters.shape[0] if parameters.ndim > 1 else 1
        return int(_call("IterativeSolverEndIteration", nbuffer, _d(_flat(parameters)), _d(_flat(residual)),
                         int(sync)))

    def add_p(self, pvectors, pp, parameters, action, apply_p, sync=True):
        """P space from sparse vectors [{index: coefficient}], the P-P action matrix `pp` (nP x nP)
        and a callback apply_p(p_coefficients (nvec x nP), actions_local, ranges) that adds the P
        contributions to this rank's range of the action rows (reference IterativeSolverAddP)."""
        self._check_top()
        offsets = np.zeros(len(pvectors) + 1, dtype=np.uint64)
        idx, coef = [], []
        for k, p in enumerate(pvectors):
            for i in sorted(p):
                idx.append(i)
                coef.append(p[i])
            offsets[k + 1] = len(idx)
        idx = np.array(idx, dtype=np.uint64)
        coef = np.array(coef, dtype=np.float64)
        ppm = np.ascontiguousarray(pp, dtype=np.float64)
        n, nP = self.n, len(pvectors)

        def tramp(pbuf, gbuf, nvec, ranges):
            pc = np.ctypeslib.as_array(pbuf, shape=(nvec * nP,)).reshape(nvec, nP)
            rg = np.ctypeslib.as_array(ranges, shape=(2 * nvec,)).reshape(nvec, 2).astype(np.int64)
            # gbuf points at element range[0] of action row 0; rows are n apart.
            g = np.ctypeslib.as_array(gbuf, shape=((nvec - 1) * n + (rg[-1, 1] - rg[-1, 0]),))
            apply_p(pc, g, rg)

        self._apply_p = APPLY_P(tramp)  # keep alive for the solver's lifetime
        nbuffer = parameters.shape[0] if parameters.ndim > 1 else 1
        self._refine_ctx = None
        r = int(_call("IterativeSolverAddP", nbuffer, nP, offsets.ctypes.data_as(PZ), idx.ctypes.data_as(PZ),
                      _d(coef), _d(ppm), _d(_flat(parameters)), _d(_flat(action)), int(sync), self._apply_p))
        self._reraise_refine()
        return r

    @property
    def end_iteration_needed(self):
        self._check_top()
        return _call("IterativeSolverEndIterationNeeded") != 0

    @property
    def errors(self):
        self._check_top()
        e = np.zeros(self.nroot)
        _call("IterativeSolverErrors", _d(e))
        return e

    def working_set_eigenvalues(self, nwork):
        self._check_top()
        ev = np.zeros(max(1, self.nroot))
        _call("IterativeSolverWorkingSetEigenvalues", _d(ev))
        return ev[:nwork]

    def statistics(self):
        self._check_top()
        return statistics()

    def solve(self, parameters, actions, problem, generate_initial_guess=False, max_iter=None):
        """One-call driver over the reverse-communication API, the loop of the reference's
        IterativeSolver.solve (iterative_solver_extension.pyx:78-165)."""
        self._check_top()
        if _device_pair(self, parameters, actions) is not None:
            return self._solve_device(parameters, actions, problem, generate_initial_guess, max_iter)
        if parameters.ndim < 2 or actions.ndim < 2:
            return self.solve(parameters.reshape([self.nroot, self.n]), actions.reshape([self.nroot, self.n]), problem,
                              generate_initial_guess, max_iter)
        nbuffer = parameters.shape[0]
        ev = np.zeros(self.nroot)
        errors = np.zeros(self.nroot)
        verbosity = _call("IterativeSolverVerbosity")
        use_diagonals = problem.diagonals(actions.reshape([actions.size]))
        if max_iter is not None:
            _call("IterativeSolverSetMaxIter", int(max_iter))
        if use_diagonals:
            _call("IterativeSolverSetDiagonals", _d(actions))
        if generate_initial_guess:
            parameters[:, :] = 0
            if isinstance(self, LinearEigensystem):
                if not use_diagonals:
                    raise ValueError("Default initial guess requested, but diagonal elements are not available")
                _call("IterativeSolverDiagonals", _d(actions))
                for i in range(self.nroot):
                    argmin = int(np.argmin(actions[0, :]))
                    actions[0, argmin] = sys.float_info.max
                    parameters[i, argmin] = 1.0
            elif isinstance(self, LinearEquations):
                for i in range(self.nroot):
                    parameters[i, i] = 1
        nwork = nbuffer
        value = None
        if getattr(self, "_refines", False):  # refined mode: the problem's action forms the refined residuals,
            self.set_refine_action(problem.action)  # and the guess is rounded to what the Q space will store
            self.quantise(parameters)
        for it in range(_call("IterativeSolverMaxIter")):
            if _call("IterativeSolverNonLinear") > 0:
                value = problem.residual(parameters.reshape([parameters.shape[-1]]),
                                         actions.reshape([parameters.shape[-1]]))
                if isinstance(self, Optimize):
                    nwork = self.add_value(value, parameters, actions)
                else:
                    nwork = self.add_vector(parameters[0, :], actions[0, :])
            else:
                problem.action(parameters, actions)
                nwork = self.add_vector(parameters[:nwork, :], actions[:nwork, :])
            while self.end_iteration_needed:
                if nwork > 0:
                    _call("IterativeSolverWorkingSetEigenvalues", _d(ev))
                    if use_diagonals:
                        _call("IterativeSolverDiagonals", _d(parameters))
                        problem.precondition(actions[:nwork, :], shift=ev[:nwork],
                                             diagonals=parameters.reshape([parameters.size])[:parameters.shape[-1]])
                    else:
                        problem.precondition(actions[:nwork, :], shift=ev[:nwork])
                nwork = self.end_iteration(parameters, actions)
            _call("IterativeSolverErrors", _d(errors))
            self.value = _call("IterativeSolverValue")
            if _call("IterativeSolverHasValues") != 0:
                reported = problem.report(it + 1 if nwork > 0 else 0, verbosity, errors, value=value)
            elif _call("IterativeSolverHasEigenvalues") != 0:
                _call("IterativeSolverEigenvalues", _d(ev))
                reported = problem.report(it + 1 if nwork > 0 else 0, verbosity, errors, eigenvalues=ev[:self.nroot])
            else:
                reported = problem.report(it + 1 if nwork > 0 else 0, verbosity, errors)
            if not reported and verbosity >= 2:
                print("Iteration", it, "log10(|residual|)=", np.log10(errors))
            if nwork < 1:
                break

    def _solve_device(self, parameters, actions, problem, generate_initial_guess, max_iter):
        """solve() on device arrays (subspace_hip.DeviceRows of this rank's range): the same loop, with no
        host copy of any vector.  problem.action / residual / diagonals receive device arrays (DeviceRows;
        residual and diagonals one DeviceVector each), and Problem.precondition's default is
        Context.precondition on the working rows with the working-set eigenvalues and the diagonals.
        The default initial guess takes the nroot smallest diagonals with Context.select and writes unit
        vectors with the sparse copy; select breaks a tie between equal diagonals towards the LARGER index,
        where the host loop's argmin takes the first.  Rows must be 16-byte aligned (an even ld)."""
        ctx = _ctx
        if ctx is None or parameters.ctx is not ctx or actions.ctx is not ctx:
            raise ValueError("solve() on device arrays: the arrays belong to the context given to use_context()")
        if not hasattr(parameters, "m"):  # one DeviceVector each: one row
            from subspace_hip import DeviceRows

            parameters = DeviceRows(ctx, 1, parameters.n, ptr=parameters.ptr)
            actions = DeviceRows(ctx, 1, actions.n, ptr=actions.ptr)
        nbuffer = parameters.m
        ev = np.zeros(self.nroot)
        errors = np.zeros(self.nroot)
        verbosity = _call("IterativeSolverVerbosity")
        use_diagonals = problem.diagonals(actions.row(0))
        if max_iter is not None:
            _call("IterativeSolverSetMaxIter", int(max_iter))
        if use_diagonals:
            _dcall("IterativeSolverHbmSetDiagonalsDevice", actions.ptr)
        if generate_initial_guess:
            guess = []
            if isinstance(self, LinearEigensystem):
                if not use_diagonals:
                    raise ValueError("Default initial guess requested, but diagonal elements are not available")
                _dcall("IterativeSolverHbmDiagonalsDevice", actions.ptr)
                idx, val = ctx.select(actions.row(0), self.nroot, offset=self.offset)
                guess = [int(idx[k]) for k in np.argsort(val, kind="stable")]  # smallest diagonal first
            elif isinstance(self, LinearEquations):
                guess = list(range(self.nroot))
            for i in range(nbuffer):  # zero, then the unit entry where this rank holds it
                ctx.sparse_copy(parameters.row(i), guess[i:i + 1], [1.0] * len(guess[i:i + 1]), offset=self.offset)
        nwork = nbuffer
        value = None
        if getattr(self, "_refines", False):  # as the host loop
            self.set_refine_action(problem.action)
            self.quantise(parameters)
        for it in range(_call("IterativeSolverMaxIter")):
            if _call("IterativeSolverNonLinear") > 0:
                value = problem.residual(parameters.row(0), actions.row(0))
                if isinstance(self, Optimize):
                    nwork = self.add_value(value, parameters, actions)
                else:
                    nwork = self.add_vector(parameters.row(0), actions.row(0))
            else:
                problem.action(parameters, actions)
                nwork = self.add_vector(parameters.head(nwork), actions.head(nwork))
            while self.end_iteration_needed:
                if nwork > 0:
                    _call("IterativeSolverWorkingSetEigenvalues", _d(ev))
                    if use_diagonals:
                        # as the host loop: the diagonals pass through the first parameter row
                        _dcall("IterativeSolverHbmDiagonalsDevice", parameters.ptr)
                        problem.precondition(actions.head(nwork), shift=ev[:nwork], diagonals=parameters.row(0))
                    else:
                        problem.precondition(actions.head(nwork), shift=ev[:nwork])
                nwork = self.end_iteration(parameters, actions)
            _call("IterativeSolverErrors", _d(errors))
            self.value = _call("IterativeSolverValue")
            if _call("IterativeSolverHasValues") != 0:
                reported = problem.report(it + 1 if nwork > 0 else 0, verbosity, errors, value=value)
            elif _call("IterativeSolverHasEigenvalues") != 0:
                _call("IterativeSolverEigenvalues", _d(ev))
                reported = problem.report(it + 1 if nwork > 0 else 0, verbosity, errors, eigenvalues=ev[:self.nroot])
            else:
                reported = problem.report(it + 1 if nwork > 0 else 0, verbosity, errors)
            if not reported and verbosity >= 2:
                print("Iteration", it, "log10(|residual|)=", np.log10(errors))
            if nwork < 1:
                break


_m_mpicomm_compute = None


def _mpicomm_compute():
    global _m_mpicomm_compute
    if _m_mpicomm_compute is None:
        _m_mpicomm_compute = int(_call("IterativeSolver_mpicomm_global"))
    return _m_mpicomm_compute


def _comm(mpicomm):
    return int(mpicomm) if mpicomm is not None else _mpicomm_compute()


def _range_arrays(range):
    rb = C.c_size_t(range[0] if range is not None else 0)
    re = C.c_size_t(range[1] if range is not None else 0)
    return rb, re


class LinearEigensystem(IterativeSolver):
    def __init__(self, n, nroot, range=None, thresh=1e-10, thresh_value=1e50, hermitian=False, verbosity=0,
                 pname="", mpicomm=None, algorithm="", options=""):
        super().__init__(n, nroot)
        rb, re = _range_arrays(range)
        _call("IterativeSolverLinearEigensystemInitialize", n, nroot, C.byref(rb), C.byref(re), thresh, thresh_value,
              1 if hermitian else 0, verbosity, pname.encode(), _comm(mpicomm), algorithm.encode(),
              options.encode())
        self._register()
        self._register_range(rb, re)
        if range is not None:
            range[0], range[1] = rb.value, re.value
        # solve() gives the refined mode (Q_REFINE=1) the problem's action and a rounded initial guess
        self._refines = (_option(options, "Q_REFINE") or "0").upper() in ("1", "T", "TRUE")

    @property
    def eigenvalues(self):
        self._check_top()
        e = np.zeros(self.nroot)
        _call("IterativeSolverEigenvalues", _d(e))
        return e


class NonLinearEquations(IterativeSolver):
    def __init__(self, n, range=None, thresh=1e-10, verbosity=0, pname="", mpicomm=None, algorithm="", options=""):
        super().__init__(n)
        rb, re = _range_arrays(range)
        _call("IterativeSolverNonLinearEquationsInitialize", n, C.byref(rb), C.byref(re), thresh, verbosity,
              pname.encode(), _comm(mpicomm), algorithm.encode(), options.encode())
        self._register()
        self._register_range(rb, re)
        if range is not None:
            range[0], range[1] = rb.value, re.value


class LinearEquations(IterativeSolver):
    def __init__(self, rhs, range=None, aughes=0.0, thresh=1e-10, thresh_value=1e50, hermitian=False, verbosity=0,
                 pname="", mpicomm=None, algorithm="", options=""):
        n = rhs.shape[-1]
        nroot = rhs.shape[0] if rhs.ndim > 1 else 1
        super().__init__(n, nroot)
        rb, re = _range_arrays(range)
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        _call("IterativeSolverLinearEquationsInitialize", n, nroot, C.byref(rb), C.byref(re), _d(r), aughes, thresh,
              thresh_value, 1 if hermitian else 0, verbosity, pname.encode(), _comm(mpicomm), algorithm.encode(),
              options.encode())
        self._register()
        self._register_range(rb, re)
        # solve() gives the refined mode (Q_STORAGE=f32,Q_REFINE=1) the problem's action, as LinearEigensystem's
        self._refines = (_option(options, "Q_REFINE") or "0").upper() in ("1", "T", "TRUE")


class Optimize(IterativeSolver):
    def __init__(self, n, range=None, thresh=1e-10, thresh_value=1e50, verbosity=0, minimize=True, pname="",
                 mpicomm=None, algorithm="", options=""):
        super().__init__(n)
        rb, re = _range_arrays(range)
        _call("IterativeSolverOptimizeInitialize", n, C.byref(rb), C.byref(re), thresh, thresh_value, verbosity,
              1 if minimize else 0, pname.encode(), _comm(mpicomm), algorithm.encode(), options.encode())
        self._register()
        self._register_range(rb, re)
