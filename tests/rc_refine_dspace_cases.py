"""The refined mode of the reverse-communication API under a Q-space limit (Q_REFINE=1, Q_REFINE_DSPACE=1,
MAX_SIZE_QSPACE), shared by tests/test_rc_refine_dspace_emul.py (the CPU emulation of the f64 C ABI) and
tests/test_q32_refined_dspace_gpu.py (the HIP library).  The loop is tests/rc_refine_cases.py's; the refine
action's log tells which of its calls came from inside end_iteration (the D-space rebuilds)."""
import numpy as np

import rc_refine_cases as rc


class Phase:
    """A solver-like (a solver, ViaDevice or Recorded over one) that notes which staging call is running, so
    that a refine action can tell the calls made from inside end_iteration."""

    def __init__(self, target):
        self.t, self.now = target, None

    def __getattr__(self, name):
        f = getattr(self.t, name)
        if name not in ("add_vector", "end_iteration"):
            return f

        def call(*args, **kw):
            self.now = name
            try:
                return f(*args, **kw)
            finally:
                self.now = None

        return call


def loop(rec, nroot, n, apply, diag, guess, max_iter=100):
    """rc.loop_refined with every call of the refine action attributed to the staging call it came from.
    -> (x, g, nwork, the RefineAction, the action's sizes inside end_iteration)."""
    ph = Phase(rec)
    inside = []

    def counted(x):
        if ph.now == "end_iteration":
            inside.append(x.shape[0])
        return apply(x)

    x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
    act = rc.RefineAction(counted, getattr(rec, "log", None))
    rec.set_refine_action(act)
    for k, i in enumerate(guess):
        x[k, i] = 1.0
    nwork = nroot
    for _ in range(max_iter):
        g[:nwork] = apply(x[:nwork])
        nwork = ph.add_vector(x[:nwork], g[:nwork])
        if nwork == 0:
            break
        ev = rec.working_set_eigenvalues(nwork)
        for k in range(nwork):
            g[k] = g[k] / ((diag - ev[k]) + 1e-15)
        nwork = ph.end_iteration(x, g)
        if nwork == 0:
            break
    return x, g, nwork, act, inside


def plain_loop(solver, nroot, n, apply, diag, guess, max_iter=100):
    """The same loop on a solver without the refined mode; -> nwork at the end."""
    x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
    for k, i in enumerate(guess):
        x[k, i] = 1.0
    nwork = nroot
    for _ in range(max_iter):
        g[:nwork] = apply(x[:nwork])
        nwork = solver.add_vector(x[:nwork], g[:nwork])
        if nwork == 0:
            break
        ev = solver.working_set_eigenvalues(nwork)
        for k in range(nwork):
            g[k] = g[k] / ((diag - ev[k]) + 1e-15)
        nwork = solver.end_iteration(x, g)
        if nwork == 0:
            break
    return nwork
