"""Host route against device route of the reverse-communication API, shared by tests/test_device_api_gpu.py
(the HIP library) and tests/test_device_api_emul.py (the CPU emulation of the f64 C ABI, where "device"
memory is host memory and the C layer's row-by-row fallback runs).

One solver instance is active at a time (the C layer drives the top of its stack), so the two routes run one
after the other through the SAME loop on numpy arrays: `Recorded` logs every staging call -- its return
value, the errors, the working-set eigenvalues, IterativeSolverHbmStatistics and every row of both arrays --
and `assert_same_log` compares the two logs entry by entry, bit for bit.  Nothing looser is justified: both
routes run the same solver call on staging vectors that hold the same bits.

`ViaDevice` is the device route behind the host calls' signature: it copies the numpy rows into
subspace_hip.DeviceRows (leading dimension ld; default: the range rounded up to even, every row 16-byte
aligned; an odd ld puts every other row at 8 mod 16), makes the device call and copies the rows back, so that the loops of tests/rc_problems.py drive either route."""
import numpy as np

import iterative_solver
import subspace_hip as sh

BIG = 1.7976931348623157e308


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class ViaDevice:
    def __init__(self, solver, ctx, ld=None, comm=None):
        self.s, self.ctx, self.comm = solver, ctx, comm
        self.off, self.local = solver.offset, solver.local
        self.ld = ld

    def __getattr__(self, name):  # everything that stages nothing: errors, eigenvalues, statistics, add_p, ...
        return getattr(self.s, name)

    def _up(self, a):
        a2 = a.reshape(-1, a.shape[-1])
        rows = sh.DeviceRows(self.ctx, a2.shape[0], self.local, self.ld)
        rows.upload(a2[:, self.off:self.off + self.local])
        return rows

    def _down(self, rows, a):
        a2 = a.reshape(-1, a.shape[-1])
        a2[:, self.off:self.off + self.local] = rows.numpy()
        if self.comm is not None and self.comm.nranks > 1:  # what sync does for the host arrays
            for k in range(a2.shape[0]):
                parts = self.comm.allgather(a2[k, self.off:self.off + self.local].tobytes())
                a2[k] = np.concatenate([np.frombuffer(p, dtype=np.float64) for p in parts])
        rows.free()

    def _staged(self, call, x, g):
        px, pg = self._up(x), self._up(g)
        r = call(px, pg)
        self._down(px, x)
        self._down(pg, g)
        return r

    def add_vector(self, x, g):
        return self._staged(self.s.add_vector, x, g)

    def end_iteration(self, x, g):
        return self._staged(self.s.end_iteration, x, g)

    def add_value(self, value, x, g):
        return self._staged(lambda px, pg: self.s.add_value(value, px, pg), x, g)

    def solution(self, roots, x, g):
        return self._staged(lambda px, pg: self.s.solution(roots, px, pg), x, g)


class Recorded:
    """`target` (a solver, or ViaDevice over it) with a log entry after every call that stages R."""

    STAGING = ("add_vector", "end_iteration", "add_value", "solution", "add_p")

    def __init__(self, target, solver, log):
        self.t, self.s, self.log = target, solver, log

    def __getattr__(self, name):
        f = getattr(self.t, name)
        if name not in self.STAGING:
            return f

        def call(*args, **kw):
            r = f(*args, **kw)
            lo, hi = self.s.offset, self.s.offset + self.s.local
            arrays = [a.reshape(-1, a.shape[-1])[:, lo:hi].copy() for a in args
                      if isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape[-1] == self.s.n]
            self.log.append((name, r, self.s.errors.copy(), self.s.working_set_eigenvalues(self.s.nroot).copy(),
                             self.s.statistics(), arrays))
            return r

        return call


def assert_same_log(host, dev):
    assert len(host) == len(dev), (len(host), len(dev))
    for i, (h, d) in enumerate(zip(host, dev)):
        where = (i, h[0])
        assert h[0] == d[0] and h[1] == d[1], (where, h[1], d[1])
        assert np.array_equal(bits(h[2]), bits(d[2])), (where, "errors", h[2], d[2])
        assert np.array_equal(bits(h[3]), bits(d[3])), (where, "working-set eigenvalues", h[3], d[3])
        assert h[4] == d[4], (where, h[4], d[4])
        assert len(h[5]) == len(d[5]) and len(h[5]) >= 2, where
        for j, (a, b) in enumerate(zip(h[5], d[5])):
            assert a.shape == b.shape, (where, j)
            for k in range(a.shape[0]):
                assert np.array_equal(bits(a[k]), bits(b[k])), (where, "array", j, "row", k)


def both_routes(make_solver, loop, ctx, ld=None, comm=None):
    """Runs loop(solver-like) through the host calls, then on a fresh instance through the device calls;
    returns (host log, device log, host result, device result)."""
    out = []
    for device in (False, True):
        log = []
        solver = make_solver()
        target = ViaDevice(solver, ctx, ld, comm) if device else solver
        try:
            res = loop(Recorded(target, solver, log))
        finally:
            solver.finalize()
        out.append((log, res))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def loop_davidson(solver, nroot, n, action, diag, guess, max_iter=40, solution=True):
    """The reverse-communication loop of a linear solver (eigenproblem or equations): action, add_vector,
    the C++ default preconditioner g / ((d - shift) + 1e-15) on the working set, end_iteration; at the
    end the solution and residual of every root."""
    x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
    for k, i in enumerate(guess):
        x[k, i] = 1.0
    nwork = nroot
    for _ in range(max_iter):
        g[:nwork] = action(x[:nwork])
        nwork = solver.add_vector(x[:nwork], g[:nwork])
        if nwork == 0:
            break
        ev = solver.working_set_eigenvalues(nwork)
        for k in range(nwork):
            g[k] = g[k] / ((diag - ev[k]) + 1e-15)
        nwork = solver.end_iteration(x, g)
        if nwork == 0:
            break
    if solution:
        solver.solution(list(range(nroot)), x, g)
    return x, g


def eigen_solver(n, nroot, **kw):
    return lambda: iterative_solver.LinearEigensystem(n, nroot, thresh=1e-8, thresh_value=BIG, hermitian=True, **kw)
