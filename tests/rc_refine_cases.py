"""The refined mode of the reverse-communication API (Q_REFINE=1, with Q_STORAGE=f64 or f32), shared by
tests/test_rc_refine_emul.py (the CPU emulation of the f64 C ABI) and tests/test_rc_q32_gpu.py (the HIP library).

The loop is tests/device_api_cases.py's loop_davidson with a refine action set on the solver first.  The action
counts its invocations and, given the log of a `Recorded`, adds an entry per invocation in the layout
assert_same_log compares -- the solutions it was given and the actions it returned -- so that the host route
and the device route are compared through the refinements too, bit for bit."""
import numpy as np

import device_api_cases as dc
import iterative_solver

EPS = float(np.finfo(np.float64).eps)


def eigen_solver(n, nroot, thresh, options):
    return lambda: iterative_solver.LinearEigensystem(n, nroot, thresh=thresh, thresh_value=dc.BIG, hermitian=True,
                                                      options=options)


class RefineAction:
    """fn(parameters, action) over numpy views (a host call) or DeviceRows (a device call): the same numpy
    work on the rows either way.  `apply` maps an (m, n) array to its action."""

    def __init__(self, apply, log=None):
        self.apply, self.log = apply, log
        self.sizes, self.q_creations = [], []

    def __call__(self, x, a):
        host = isinstance(x, np.ndarray)
        xv = x if host else x.numpy()
        av = self.apply(xv)
        if host:
            a[:, :] = av
        else:
            a.upload(av)
        self.sizes.append(xv.shape[0])
        self.q_creations.append(iterative_solver.statistics()["q_creations"])
        if self.log is not None:
            self.log.append(("refine", xv.shape[0], np.zeros(0), np.zeros(0), None, [xv.copy(), np.array(av)]))


def loop_refined(rec, nroot, n, apply, diag, guess, max_iter=60, refine=True):
    """-> (x, g, nwork at the end, the RefineAction).  rec: a solver, or device_api_cases.Recorded over one."""
    act = RefineAction(apply, getattr(rec, "log", None))
    if refine:
        rec.set_refine_action(act)
    x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
    for k, i in enumerate(guess):
        x[k, i] = 1.0
    nwork = nroot
    for _ in range(max_iter):
        g[:nwork] = apply(x[:nwork])
        nwork = rec.add_vector(x[:nwork], g[:nwork])
        if nwork == 0:
            break
        ev = rec.working_set_eigenvalues(nwork)
        for k in range(nwork):
            g[k] = g[k] / ((diag - ev[k]) + 1e-15)
        nwork = rec.end_iteration(x, g)
        if nwork == 0:
            break
    return x, g, nwork, act


def result(solver, nroot, n, h, threshold, nwork):
    """The layout test_q32_refined_gpu.refined_criteria reads, from a finished reverse-communication loop
    (nwork: its last working-set size): residual_norms are |H x - theta x| recomputed in numpy from solution()."""
    x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
    errors = solver.errors.copy()
    ev = solver.eigenvalues.copy()
    solver.solution(list(range(nroot)), x, g)
    norms = np.array([np.linalg.norm(x[k] @ h - ev[k] * x[k]) for k in range(nroot)])
    return {"converged": bool(nwork == 0 and np.all(errors <= threshold)), "errors": errors, "eigenvalues": ev,
            "residual_norms": norms, "iterations": solver.statistics()["iterations"], "solutions": x,
            "refine": solver.refine_statistics()}


def stored(diag):
    """The diagonal as an f32 Q space holds it.  A loop on a Q_STORAGE=f32 instance preconditions with it, as
    the C++ solve() does (it keeps the problem's diagonals in a Q vector, and IterativeSolverSetDiagonals on
    such an instance does the same): with actions stored rounded, the residual of a unit-vector guess is
    rounding noise at the guess's index, eps32 |a| and not the exact zero of f64 arithmetic, and the
    preconditioner's (d - theta) + 1e-15 must then not be an exact zero either."""
    return np.asarray(diag).astype(np.float32).astype(np.float64)


def norm2(h):
    return float(np.max(np.abs(np.linalg.eigvalsh((h + h.T) / 2))))
