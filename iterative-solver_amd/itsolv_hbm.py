"""ctypes binding of libitsolv_hbm.so (C ABI: include/itsolv_hbm.h): the restated Davidson / DIIS
solvers running over the HBM handlers.  The options / result structures are shared with the
oracle's CPU twin (oracle/itsolv_oracle.cpp)."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

import subspace_hip as sh

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libitsolv_hbm.so")
MAX_ROOTS = 64
TRACE_ITER, TRACE_ROOTS = 256, 8

EXPORTS = [
    "itsolv_last_error", "itsolv_default_options", "itsolv_davidson_synthetic", "itsolv_davidson_dense",
    "itsolv_diis_synthetic", "itsolv_diis_dense", "itsolv_linear_equations_dense", "itsolv_optimize_dense",
    "itsolv_davidson_synth", "itsolv_diis_synth",
    # Davidson with the Q space stored in f32 (itsolv_hbm/hbm_vec_f32.h)
    "itsolv_davidson_dense_q32", "itsolv_davidson_synth_q32",
    # the same in the refined mode (f64 thresholds), and what the last refined solve spent
    "itsolv_davidson_dense_q32_refined", "itsolv_davidson_synth_q32_refined", "itsolv_q32_refine_stats",
    # the refined mode under a Q-space limit (a consistent D space), and what it spent on the D space
    "itsolv_davidson_dense_q32_refined_dspace", "itsolv_davidson_synth_q32_refined_dspace", "itsolv_q32_dspace_stats",
    # linear equations on the synthetic H (f64), and dense / synthetic over the f32 Q space, plain and refined
    "itsolv_linear_equations_synth",
    "itsolv_linear_equations_dense_q32", "itsolv_linear_equations_synth_q32",
    "itsolv_linear_equations_dense_q32_refined", "itsolv_linear_equations_synth_q32_refined",
    # DIIS with its history stored as f32 differences behind f64 anchors, and what the last such solve held
    "itsolv_diis_synth_q32", "itsolv_diis_dense_q32", "itsolv_q32_diis_stats",
]
# Linear equations over the f32 Q space: absent from the CPU emulation of the library, as the sets below; a set
# of their own (those stay what they were).
OPTIONAL_LINEQ = frozenset(n for n in EXPORTS if n.startswith("itsolv_linear_equations_") and "_q32" in n)
# Absent from the CPU emulation of the library (loaded through this binding by patching LIB_PATH).
# DIIS over f32 differences: absent from the emulation in the same way; again a set of its own.
OPTIONAL_DIIS = frozenset(n for n in EXPORTS if n.startswith("itsolv_diis_") and n.endswith("_q32")) | {"itsolv_q32_diis_stats"}
OPTIONAL = frozenset(n for n in EXPORTS if n.endswith("_q32")) - OPTIONAL_LINEQ - OPTIONAL_DIIS
# The refined mode's entry points, optional in the same way; a set of their own: OPTIONAL stays the plain f32 Q space.
OPTIONAL_REFINED = (frozenset(n for n in EXPORTS if n.endswith("_q32_refined") or n == "itsolv_q32_refine_stats")
                    - OPTIONAL_LINEQ)
# The refined mode's consistent D space, optional in the same way; again a set of its own.
OPTIONAL_DSPACE = frozenset(n for n in EXPORTS if n.endswith("_q32_refined_dspace") or n == "itsolv_q32_dspace_stats")

# Diagonal families of the synthetic H (include/subspace_hip.h sspx_synth, itsolv_hbm/problems.h).
DIAG_LINEAR, DIAG_BOUNDED = 0, 1


class Synth(C.Structure):
    _fields_ = [("rho", C.c_double), ("rank", C.c_int), ("seed", C.c_ulonglong), ("diag_kind", C.c_int),
                ("alpha", C.c_double), ("target", C.c_double)]


def c5_spec(n: int, rank: int = 1, seed: int = 3, alpha: float = 0.2) -> dict:
    """BASELINE config C5's well-posed DIIS instance (itsolv_hbm/problems.h c5_spec): r = H (x - t 1),
    H = diag(1 + 2 frac(g phi1)) + (1/n) sum_l u_l u_l^T, preconditioner diagonal mismatched by alpha,
    t = 1/sqrt(n) (a unit-norm solution).  Keyword arguments of diis_synthetic / oracle.diis_synthetic."""
    return dict(rho=1.0 / n, rank=rank, seed=seed, diag_kind=DIAG_BOUNDED, alpha=alpha, target=1.0 / math.sqrt(n))


class Refine(C.Structure):
    """itsolv_q32_refine: kappa <= 0 means the default of 8."""
    _fields_ = [("kappa", C.c_double)]


class Options(C.Structure):
    _fields_ = [
        ("nroots", C.c_int),
        ("nwork", C.c_int),
        ("max_iter", C.c_int),
        ("max_size_qspace", C.c_int),
        ("reset_D", C.c_int),
        ("reset_D_max_Q_size", C.c_int),
        ("max_p", C.c_int),
        ("p_threshold", C.c_double),
        ("convergence_threshold", C.c_double),
        ("hermitian", C.c_int),
        ("generate_initial_guess", C.c_int),
        ("verbosity", C.c_int),
        ("augmented_hessian", C.c_double),
        ("block_gram_schmidt", C.c_int),
    ]


class Result(C.Structure):
    _fields_ = [
        ("converged", C.c_int),
        ("iterations", C.c_int),
        ("r_creations", C.c_int),
        ("q_creations", C.c_int),
        ("nroots", C.c_int),
        ("eigenvalues", C.c_double * MAX_ROOTS),
        ("errors", C.c_double * MAX_ROOTS),
        ("residual_norms", C.c_double * MAX_ROOTS),
        ("seconds", C.c_double),
        ("n_eig_trace", C.c_int),
        ("eig_trace", C.c_double * 256),
        ("trace_roots", C.c_int),
        ("trace_nq", C.c_int * TRACE_ITER),
        ("trace_nwork", C.c_int * TRACE_ITER),
        ("trace_eigenvalues", C.c_double * (TRACE_ITER * TRACE_ROOTS)),
        ("trace_errors", C.c_double * (TRACE_ITER * TRACE_ROOTS)),
        ("redundant_params", C.c_int),
        ("null_params", C.c_int),
        ("trace_screened", C.c_int * TRACE_ITER),
        ("host_algebra_seconds", C.c_double),
        ("host_algebra_calls", C.c_int),
        ("host_algebra_max_dim", C.c_int),
    ]

    def as_dict(self):
        k = self.nroots
        return {
            "converged": bool(self.converged),
            "iterations": self.iterations,
            "r_creations": self.r_creations,
            "q_creations": self.q_creations,
            "redundant_params": self.redundant_params,
            "null_params": self.null_params,
            "eigenvalues": np.array(self.eigenvalues[:k]),
            "errors": np.array(self.errors[:k]),
            "residual_norms": np.array(self.residual_norms[:k]),
            "seconds": self.seconds,
            "host_algebra": {"seconds": self.host_algebra_seconds, "calls": self.host_algebra_calls,
                             "max_dim": self.host_algebra_max_dim},
            "eig_trace": np.array(self.eig_trace[: self.n_eig_trace]),
            "trace": self.trace(),
        }

    def trace(self):
        """Per-iteration parity observables: one entry per solve() iteration."""
        it, nr = self.n_eig_trace, self.trace_roots
        ev = np.array(self.trace_eigenvalues[: it * TRACE_ROOTS]).reshape(it, TRACE_ROOTS)[:, :nr]
        er = np.array(self.trace_errors[: it * TRACE_ROOTS]).reshape(it, TRACE_ROOTS)[:, :nr]
        return {"eigenvalues": ev, "errors": er, "nq": np.array(self.trace_nq[:it]),
                "nwork": np.array(self.trace_nwork[:it]), "screened": np.array(self.trace_screened[:it])}


def make_options(**kw) -> Options:
    o = Options(nroots=1, nwork=0, max_iter=100, max_size_qspace=0, reset_D=0, reset_D_max_Q_size=0, max_p=0,
                p_threshold=0.0, convergence_threshold=1e-8, hermitian=1, generate_initial_guess=1, verbosity=0,
                augmented_hessian=0.0, block_gram_schmidt=-1)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


_lib = None


def load_library():
    global _lib
    if _lib is None:
        sh.load_library()  # libsubspace_hip.so first (dependency, RTLD_GLOBAL)
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} missing: run `make -C iterative-solver_amd`")
        L = C.CDLL(LIB_PATH)
        P, Z, D, I, U = C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_ulonglong
        PO, PR, PD = C.POINTER(Options), C.POINTER(Result), C.POINTER(C.c_double)
        PF, PI = C.POINTER(Refine), C.POINTER(C.c_int)
        sig = {
            "itsolv_last_error": (C.c_char_p, []),
            "itsolv_default_options": (None, [PO]),
            "itsolv_davidson_synthetic": (I, [P, Z, D, I, U, PO, PR, PD]),
            "itsolv_davidson_dense": (I, [P, PD, Z, PO, PR, PD]),
            "itsolv_diis_synthetic": (I, [P, Z, D, I, U, PO, PR, PD]),
            "itsolv_diis_dense": (I, [P, PD, Z, PO, PR, PD]),
            "itsolv_linear_equations_dense": (I, [P, PD, Z, PD, I, PO, PR, PD]),
            "itsolv_optimize_dense": (I, [P, PD, Z, I, PO, PR, PD]),
            "itsolv_davidson_synth": (I, [P, Z, C.POINTER(Synth), PO, PR, PD]),
            "itsolv_diis_synth": (I, [P, Z, C.POINTER(Synth), PO, PR, PD]),
            "itsolv_davidson_dense_q32": (I, [P, PD, Z, PO, PR, PD]),
            "itsolv_davidson_synth_q32": (I, [P, Z, C.POINTER(Synth), PO, PR, PD]),
            "itsolv_davidson_dense_q32_refined": (I, [P, PD, Z, PO, PF, PR, PD]),
            "itsolv_davidson_synth_q32_refined": (I, [P, Z, C.POINTER(Synth), PO, PF, PR, PD]),
            "itsolv_q32_refine_stats": (I, [PI, PI, PD]),
            "itsolv_davidson_dense_q32_refined_dspace": (I, [P, PD, Z, PO, PF, PR, PD]),
            "itsolv_davidson_synth_q32_refined_dspace": (I, [P, Z, C.POINTER(Synth), PO, PF, PR, PD]),
            "itsolv_q32_dspace_stats": (I, [PI, PI]),
            "itsolv_linear_equations_synth": (I, [P, Z, C.POINTER(Synth), I, U, PO, PR, PD]),
            "itsolv_linear_equations_dense_q32": (I, [P, PD, Z, PD, I, PO, PR, PD]),
            "itsolv_linear_equations_synth_q32": (I, [P, Z, C.POINTER(Synth), I, U, PO, PR, PD]),
            "itsolv_linear_equations_dense_q32_refined": (I, [P, PD, Z, PD, I, PO, PF, PR, PD]),
            "itsolv_linear_equations_synth_q32_refined": (I, [P, Z, C.POINTER(Synth), I, U, PO, PF, PR, PD]),
            "itsolv_diis_synth_q32": (I, [P, Z, C.POINTER(Synth), PO, PR, PD]),
            "itsolv_diis_dense_q32": (I, [P, PD, Z, PO, PR, PD]),
            "itsolv_q32_diis_stats": (I, [PI, PI, C.POINTER(C.c_size_t)]),
        }
        optional = OPTIONAL | OPTIONAL_REFINED | OPTIONAL_DSPACE | OPTIONAL_LINEQ | OPTIONAL_DIIS
        for name, (res, args) in sig.items():
            if name in optional and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _entry(name: str, q32: bool, refine: bool = False, refine_dspace: bool = False):
    """The solver entry point `name`, or with q32 its form over a Q space stored in f32 (refine: in the
    refined mode; refine_dspace: with its consistent D space, which admits max_size_qspace)."""
    if refine and not q32:
        raise ValueError("refine=True needs q32=True: the refined mode is a mode of the f32 Q space")
    if refine_dspace and not refine:
        raise ValueError("refine_dspace=True needs refine=True: the consistent D space is part of the refined mode")
    if not q32:
        return getattr(load_library(), name)
    full = name + ("_q32_refined_dspace" if refine_dspace else "_q32_refined" if refine else "_q32")
    f = getattr(load_library(), full, None)
    if f is None:
        raise sh.SspError(7, f"{full}: the loaded library has no f32 Q space")
    return f


def _refine_args(refine: bool, kappa):
    """The extra argument of a *_q32_refined entry (none for the others)."""
    if not refine:
        if kappa is not None:
            raise ValueError("kappa is an option of refine=True")
        return ()
    return (C.byref(Refine(0.0 if kappa is None else float(kappa))),)


def _refine_stats() -> dict:
    a, f, d = C.c_int(), C.c_int(), C.c_double()
    load_library().itsolv_q32_refine_stats(C.byref(a), C.byref(f), C.byref(d))
    return {"refined_actions": a.value, "first_refined_iteration": f.value, "max_delta": d.value}


def _dspace_stats() -> dict:
    r, a = C.c_int(), C.c_int()
    load_library().itsolv_q32_dspace_stats(C.byref(r), C.byref(a))
    return {"dspace_rebuilds": r.value, "dspace_actions": a.value}


def _call(fn, args, nout):
    res = Result()
    out = np.zeros(max(1, nout))
    # nout == 0: no solution copy-back (null pointer; the C side then skips the download)
    ptr = out.ctypes.data_as(C.POINTER(C.c_double)) if nout > 0 else None
    code = fn(*args, C.byref(res), ptr)
    if code != 0:
        raise RuntimeError(f"{fn.__name__}: {load_library().itsolv_last_error().decode()}")
    return res.as_dict(), out


def davidson_synthetic(ctx: sh.Context, n: int, rho: float, rank: int, seed: int, n_local: int | None = None,
                       solutions: bool = True, *, diag_kind: int = DIAG_LINEAR, alpha: float = 0.0,
                       target: float = 1.0, q32: bool = False, refine: bool = False, kappa: float | None = None,
                       refine_dspace: bool = False, **opts):
    """q32: the Q space is stored in f32 (half the HBM and bytes of every pass over it; arithmetic in f64).
    refine (with q32): the refined mode, which reaches f64 thresholds at the price of one more action per
    refined root and iteration (include/itsolv_hbm.h); the result then has "refine" (its statistics).
    refine_dspace (with refine): the refined mode under max_size_qspace, its D space rebuilt consistently at
    nD <= nroots more actions per rebuild; the result then has "refine_dspace" (rebuilds and their actions)."""
    fn = _entry("itsolv_davidson_synth", q32, refine, refine_dspace)
    o = make_options(**opts)
    nl = n if n_local is None else n_local
    spec = Synth(rho, rank, seed, diag_kind, alpha, target)
    r, sol = _call(fn, (ctx.handle, n, C.byref(spec), C.byref(o)) + _refine_args(refine, kappa),
                   o.nroots * nl if solutions else 0)
    if refine:
        r["refine"] = _refine_stats()
    if refine_dspace:
        r["refine_dspace"] = _dspace_stats()
    if solutions:
        r["solutions"] = sol[: o.nroots * nl].reshape(o.nroots, nl)
    return r


def davidson_dense(ctx: sh.Context, h: np.ndarray, q32: bool = False, refine: bool = False,
                   kappa: float | None = None, refine_dspace: bool = False, **opts):
    """q32: the Q space is stored in f32 (arithmetic in f64); refine, refine_dspace: as davidson_synthetic's."""
    fn = _entry("itsolv_davidson_dense", q32, refine, refine_dspace)
    h = np.ascontiguousarray(h, dtype=np.float64)
    n = h.shape[0]
    o = make_options(**opts)
    r, sol = _call(fn, (ctx.handle, h.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(o))
                   + _refine_args(refine, kappa), o.nroots * n)
    if refine:
        r["refine"] = _refine_stats()
    if refine_dspace:
        r["refine_dspace"] = _dspace_stats()
    r["solutions"] = sol[: o.nroots * n].reshape(o.nroots, n)
    return r


def _diis_stats() -> dict:
    p, d, b = C.c_int(), C.c_int(), C.c_size_t()
    load_library().itsolv_q32_diis_stats(C.byref(p), C.byref(d), C.byref(b))
    return {"points": p.value, "pairs": d.value, "history_bytes": b.value}


def diis_synthetic(ctx: sh.Context, n: int, rho: float, rank: int, seed: int, n_local: int | None = None,
                   solutions: bool = True, *, diag_kind: int = DIAG_LINEAR, alpha: float = 0.0,
                       target: float = 1.0, q32: bool = False, **opts):
    """q32: the history is held as f32 differences between successive iterates behind two f64 anchors
    (include/itsolv_hbm.h itsolv_diis_synth_q32): about half the HBM of the f64 history, f64 thresholds, the
    iterations of the f64 solve; the result then has "diis_q32" (points, pairs of differences, history bytes)."""
    o = make_options(**opts)
    nl = n if n_local is None else n_local
    spec = Synth(rho, rank, seed, diag_kind, alpha, target)
    r, x = _call(_entry("itsolv_diis_synth", q32), (ctx.handle, n, C.byref(spec), C.byref(o)),
                 nl if solutions else 0)
    if q32:
        r["diis_q32"] = _diis_stats()
    if solutions:
        r["x"] = x[:nl]
    return r


def diis_dense(ctx: sh.Context, h: np.ndarray, q32: bool = False, **opts):
    """q32: as diis_synthetic's."""
    h = np.ascontiguousarray(h, dtype=np.float64)
    n = h.shape[0]
    o = make_options(**opts)
    r, x = _call(_entry("itsolv_diis_dense", q32), (ctx.handle, h.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                   C.byref(o)), n)
    if q32:
        r["diis_q32"] = _diis_stats()
    r["x"] = x[:n]
    return r


def linear_equations_dense(ctx: sh.Context, a: np.ndarray, rhs: np.ndarray, q32: bool = False, refine: bool = False,
                           kappa: float | None = None, **opts):
    """LinearEquationsDavidson on A x_r = b_r (rows of rhs); returns the result dict with "x".
    q32: the Q space (and with it the right-hand sides) stored in f32: meaningful down to about 1e-6.
    refine (with q32): the refined mode, which keeps an f64 twin of every right-hand side and reaches f64
    thresholds at one more action per refined root and iteration; the result then has "refine"."""
    fn = _entry("itsolv_linear_equations_dense", q32, refine)
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_2d(rhs), dtype=np.float64)
    n, nrhs = a.shape[0], b.shape[0]
    o = make_options(**opts)
    r, x = _call(fn, (ctx.handle, a.ctypes.data_as(C.POINTER(C.c_double)), n, b.ctypes.data_as(C.POINTER(C.c_double)),
                      nrhs, C.byref(o)) + _refine_args(refine, kappa), n * nrhs)
    if refine:
        r["refine"] = _refine_stats()
    r["x"] = x[:n * nrhs].reshape(nrhs, n)
    return r


def linear_equations_synth(ctx: sh.Context, n: int, rho: float, rank: int, seed: int, nrhs: int, rhs_seed: int,
                           n_local: int | None = None, solutions: bool = True, *, diag_kind: int = DIAG_LINEAR,
                           alpha: float = 0.0, q32: bool = False, refine: bool = False, kappa: float | None = None,
                           **opts):
    """LinearEquationsDavidson on the synthetic H (davidson_synthetic's; SPD for rho >= 0) with the right-hand
    sides b_r = fill_random(seed=rhs_seed, vec=r); q32, refine, kappa: as linear_equations_dense's.  Returns the
    result dict with "x" (nrhs x the local length) unless solutions is False."""
    fn = _entry("itsolv_linear_equations_synth", q32, refine)
    o = make_options(**opts)
    nl = n if n_local is None else n_local
    spec = Synth(rho, rank, seed, diag_kind, alpha, 1.0)
    r, x = _call(fn, (ctx.handle, n, C.byref(spec), nrhs, rhs_seed, C.byref(o)) + _refine_args(refine, kappa),
                 nrhs * nl if solutions else 0)
    if refine:
        r["refine"] = _refine_stats()
    if solutions:
        r["x"] = x[: nrhs * nl].reshape(nrhs, nl)
    return r


def optimize_dense(ctx: sh.Context, h: np.ndarray, algorithm: str = "BFGS", **opts):
    """OptimizeBFGS / OptimizeSD on the Rayleigh quotient of h from e_0 (function value in eigenvalues[0])."""
    h = np.ascontiguousarray(h, dtype=np.float64)
    n = h.shape[0]
    o = make_options(**opts)
    r, x = _call(load_library().itsolv_optimize_dense,
                 (ctx.handle, h.ctypes.data_as(C.POINTER(C.c_double)), n, 0 if algorithm == "BFGS" else 1,
                  C.byref(o)), n)
    r["x"] = x[:n]
    return r
