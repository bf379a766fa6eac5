"""The device forms of the reverse-communication API (include/iterative_solver_c.h, IterativeSolverHbm*Device)
on the GPU: two instances of the same solver on the same problem, one driven through the host calls and one
through the device calls, with the same values going in (tests/device_api_cases.py).  After every call: the
same return value, the same errors, working-set eigenvalues and IterativeSolverHbmStatistics, and every row of
both arrays equal bit for bit.  Nothing looser is justified: both routes run the same solver on staging
vectors that hold the same bits -- ssp_rows_import is a bit copy of what ssp_upload copies, ssp_rows_export
stores the product ssp_scal would have stored before ssp_download.

The CPU twin over the emulation (the C layer's fallback without ssp_rows_*): tests/test_device_api_emul.py."""
import numpy as np
import pytest

import device_api_cases as dc
import iterative_solver
import rc_problems as rp
import subspace_hip as sh
from test_python_api_gpu import hamiltonian

pytestmark = pytest.mark.gpu
RHO, RANK, SEED = 0.1, 4, 7


@pytest.fixture()
def api(ctx):
    """The C API on the session's context (the ledger and the device rows need the instance's context)."""
    iterative_solver.use_context(ctx)
    yield ctx
    iterative_solver.use_context(None)


def synthetic(ctx, n):
    """(action on numpy rows, diagonal) of the synthetic problem, the action by the library's kernel on
    aligned scratch vectors -- the same kernel on the same bits for both routes."""
    xx, yy = [], []

    def action(x):
        while len(xx) < x.shape[0]:
            xx.append(ctx.alloc(n))
            yy.append(ctx.alloc(n))
        k = x.shape[0]
        for v, row in zip(xx, x):
            ctx.upload_into(v, row)
        ctx.synthetic_action(xx[:k], yy[:k], RHO, RANK, SEED)
        return np.vstack([v.numpy() for v in yy[:k]])

    d = ctx.alloc(n)
    ctx.synthetic_diagonal(d, RHO, RANK)
    diag = d.numpy()
    d.free()

    def release():
        for v in xx + yy:
            v.free()

    return action, diag, release


@pytest.mark.parametrize("ld", [None, 29], ids=["aligned", "alternating"])
def test_linear_eigensystem_on_the_short_vector_path(api, ld):
    h = hamiltonian("bh", 1e-8)
    n, nroot = h.shape[0], 2
    d = np.diag(h).copy()
    guess = sorted(np.argsort(d, kind="stable")[:nroot])
    make = dc.eigen_solver(n, nroot, options=f"MAX_SIZE_QSPACE={6 * nroot},RESET_D=8")
    hl, dl, _, _ = dc.both_routes(make, lambda s: dc.loop_davidson(s, nroot, n, lambda x: x @ h, d, guess), api, ld=ld)
    dc.assert_same_log(hl, dl)
    assert hl[-1][0] == "solution" and np.all(hl[-1][2] < 1e-7) and len(hl) > 6


@pytest.mark.parametrize("n,nroot,ld,max_iter", [(100_003, 4, None, 40), (100_003, 4, 100_003, 40),
                                                 (2**20 + 5, 2, 2**20 + 5, 6), (2**20 + 5, 2, 2**20 + 6, 6)],
                         ids=["100003-aligned", "100003-ld=n", "2^20+5-ld=n", "2^20+5-ld=n+1"])
def test_linear_eigensystem_on_the_synthetic_problem(api, n, nroot, ld, max_iter):
    """n = 2^20 + 5: the fused solver passes (they switch on from 2^20 elements); a few iterations of it.
    An odd ld puts every other row at 8 mod 16."""
    action, diag, release = synthetic(api, n)
    make = dc.eigen_solver(n, nroot)
    loop = lambda s: dc.loop_davidson(s, nroot, n, action, diag, list(range(nroot)), max_iter=max_iter)  # noqa: E731
    hl, dl, _, _ = dc.both_routes(make, loop, api, ld=ld)
    release()
    dc.assert_same_log(hl, dl)
    assert hl[-1][0] == "solution" and len(hl) >= min(2 * max_iter, 9)
    if max_iter > 6:
        assert np.all(hl[-1][2] < 1e-7), hl[-1][2]


def test_linear_equations(api):
    h = hamiltonian("bh", 1e-8) + 3.0 * np.eye(28)
    rhs = np.vstack([h[:, 0] + 1.0, np.arange(1.0, 29.0)])
    make = lambda: iterative_solver.LinearEquations(rhs, thresh=1e-9, hermitian=True)  # noqa: E731
    loop = lambda s: dc.loop_davidson(s, 2, 28, lambda x: x @ h, np.diag(h).copy(), [0, 1])  # noqa: E731
    hl, dl, hr, _ = dc.both_routes(make, loop, api)
    dc.assert_same_log(hl, dl)
    assert np.all(hl[-1][2] < 1e-7) and np.allclose(hr[0] @ h, rhs, atol=1e-6)


@pytest.mark.parametrize("optimize", [False, True], ids=["DIIS", "Optimize"])
def test_nonlinear_solvers_on_the_quadratic_form(api, optimize):
    """NonLinearEquations through AddVectorDevice's non-linear branch, Optimize through AddValueDevice."""
    n = 20
    hq = rp.quadratic_matrix(n, 10.0)
    make = (lambda: iterative_solver.Optimize(n, thresh=1e-8)) if optimize else \
        (lambda: iterative_solver.NonLinearEquations(n, thresh=1e-8))
    hl, dl, hr, dr = dc.both_routes(make, lambda s: rp.loop_quadratic(s, hq, optimize), api)
    dc.assert_same_log(hl, dl)
    assert hr[1] == dr[1] and 3 < hr[1] < 100 and np.allclose(hr[0][-1][2], 1.0, atol=1e-6)
    assert {e[0] for e in hl} == ({"add_value", "end_iteration"} if optimize else {"add_vector", "end_iteration"})


def test_a_p_space_through_host_arrays_then_device_calls(api):
    """Mixed use: IterativeSolverAddP stays host-only, the device calls follow it on the same instance."""
    h = hamiltonian("bh", 1e-8)
    nroot, np_ = 3, 4
    make = dc.eigen_solver(h.shape[0], nroot, options=f"MAX_SIZE_QSPACE={6 * nroot},RESET_D=8")
    hl, dl, hr, dr = dc.both_routes(make, lambda s: rp.loop_eigen(s, h, nroot, np_), api)
    dc.assert_same_log(hl, dl)
    assert hr == dr and hl[0][0] == "add_p" and len(hl) > 4


@pytest.mark.parametrize("ld", [None, 4099], ids=["aligned", "alternating"])
def test_each_device_call_is_one_import_and_one_export_launch_per_array(api, ld):
    n, nroot = 4099, 3
    action, diag, release = synthetic(api, n)
    s = iterative_solver.LinearEigensystem(n, nroot, thresh=1e-8, hermitian=True)
    px, pg = sh.DeviceRows(api, nroot, n, ld), sh.DeviceRows(api, nroot, n, ld)
    x = np.zeros((nroot, n))
    x[np.arange(nroot), np.arange(nroot)] = 1.0
    px.upload(x)
    pg.upload(action(x))

    def ledger_of(call):
        api.ledger_enable(True)
        try:
            api.ledger_reset()
            r = call()
            api.synchronize()
            return r, api.ledger()
        finally:
            api.ledger_enable(False)

    nwork, led = ledger_of(lambda: s.add_vector(px, pg))
    assert nwork == nroot
    for name in ("rows_import", "rows_export"):
        assert led[name]["calls"] == 2 and led[name]["bytes"] == 2 * 16.0 * nroot * n, (name, led[name])
    nwork, led = ledger_of(lambda: s.end_iteration(px, pg))
    for name in ("rows_import", "rows_export"):
        assert led[name]["calls"] == 2, (name, led[name])
    _, led = ledger_of(lambda: s.solution([0, 1], px, pg))
    assert "rows_import" not in led and led["rows_export"]["calls"] == 2, led
    s.finalize()
    px.free()
    pg.free()
    release()


def test_diagonals_round_trip_through_device_memory(api):
    n = 4099
    s = iterative_solver.LinearEigensystem(n, 2)
    want = np.arange(float(n)) ** 2 - 0.5
    buf = api.upload(np.concatenate([[-1.0], want, [-2.0]]))
    out = api.upload(np.full(n + 2, -3.0))
    for base in (0, 1):  # 16-byte aligned, and at 8 mod 16
        api.upload_into(buf, np.concatenate([np.full(base, -1.0), want, np.full(2 - base, -2.0)]))
        iterative_solver._dcall("IterativeSolverHbmSetDiagonalsDevice", buf.ptr + 8 * base)
        host = np.zeros(n)
        iterative_solver._call("IterativeSolverDiagonals", host.ctypes.data_as(iterative_solver.PD))
        assert np.array_equal(dc.bits(host), dc.bits(want))
        iterative_solver._dcall("IterativeSolverHbmDiagonalsDevice", out.ptr + 8 * base)
        got = out.numpy()
        assert np.array_equal(dc.bits(got[base:base + n]), dc.bits(want))
        assert np.all(got[:base] == -3.0) and np.all(got[base + n:] == -3.0)
        api.upload_into(out, np.full(n + 2, -3.0))
    # set through the host call, read through the device call
    iterative_solver._call("IterativeSolverSetDiagonals", (2.0 * want).ctypes.data_as(iterative_solver.PD))
    iterative_solver._dcall("IterativeSolverHbmDiagonalsDevice", out.ptr)
    assert np.array_equal(out.numpy()[:n], 2.0 * want)
    s.finalize()
    buf.free()
    out.free()


def test_mixed_and_misshapen_arrays_are_refused(api):
    s = iterative_solver.LinearEigensystem(28, 2)
    rows = sh.DeviceRows(api, 2, 28)
    for f in (lambda: s.add_vector(np.zeros((2, 28)), rows), lambda: s.end_iteration(rows, np.zeros((2, 28))),
              lambda: s.add_value(0.0, rows.row(0), np.zeros(28)), lambda: s.solution([0], np.zeros(28), rows.row(0))):
        with pytest.raises(TypeError):
            f()
    with pytest.raises(ValueError, match="range"):
        s.add_vector(sh.DeviceRows(api, 2, 27), sh.DeviceRows(api, 2, 27))
    with pytest.raises(ValueError, match="shapes"):
        s.add_vector(rows, sh.DeviceRows(api, 1, 28))
    assert s.statistics()["iterations"] == 0
    s.finalize()
    rows.free()


class DeviceSynthetic(iterative_solver.Problem):
    """The synthetic problem on device arrays: Context.synthetic_action, synthetic_diagonal, precondition."""

    def __init__(self, ctx):
        super().__init__()
        self.ctx = ctx

    def action(self, parameters, actions):
        self.ctx.synthetic_action(parameters.rows(), actions.rows(), RHO, RANK, SEED)

    def diagonals(self, d):
        self.ctx.synthetic_diagonal(d, RHO, RANK)
        return True

    def precondition(self, residual, shift=None, diagonals=None):
        self.ctx.precondition(residual.rows(), diagonals, shift)


class HostWrapped(iterative_solver.Problem):
    """The same device problem behind numpy arrays: every method uploads, calls it and downloads, so both
    solve() loops run the same kernels on the same bits."""

    def __init__(self, dev, n):
        super().__init__()
        self.dev, self.ctx, self.n = dev, dev.ctx, n

    def _through(self, a, call, *more):
        rows = sh.DeviceRows(self.ctx, a.shape[0], self.n)
        rows.upload(a)
        call(rows, *more)
        a[:, :] = rows.numpy()
        rows.free()

    def action(self, parameters, actions):
        p = sh.DeviceRows(self.ctx, parameters.shape[0], self.n)
        p.upload(parameters)
        self._through(actions, lambda rows: self.dev.action(p, rows))
        p.free()

    def diagonals(self, d):
        v = self.ctx.alloc(self.n)
        self.dev.diagonals(v)
        d[:self.n] = v.numpy()
        v.free()
        return True

    def precondition(self, residual, shift=None, diagonals=None):
        d = self.ctx.upload(diagonals)
        self._through(residual, lambda rows: self.dev.precondition(rows, shift=shift, diagonals=d))
        d.free()


def test_python_solve_on_device_rows_is_the_host_solve(api):
    """solve() with a device Problem against the host solve() of the same problem.  The diagonal
    1 + g + rank * rho has no ties (select and argmin break ties differently)."""
    n, nroot = 20_011, 3
    dev = DeviceSynthetic(api)
    results = []
    for device in (False, True):
        s = iterative_solver.LinearEigensystem(n, nroot, thresh=1e-8, thresh_value=dc.BIG, hermitian=True)
        if device:
            x, g = sh.DeviceRows(api, nroot, n), sh.DeviceRows(api, nroot, n)
            s.solve(x, g, dev, generate_initial_guess=True)
            s.solution(list(range(nroot)), x, g)
            xs, gs = x.numpy(), g.numpy()
            x.free()
            g.free()
        else:
            xs, gs = np.zeros((nroot, n)), np.zeros((nroot, n))
            s.solve(xs, gs, HostWrapped(dev, n), generate_initial_guess=True)
            s.solution(list(range(nroot)), xs, gs)
        results.append((s.statistics(), s.eigenvalues.copy(), s.errors.copy(), xs, gs))
        s.finalize()
    (hs, he, herr, hx, hg), (ds, de, derr, dx, dg) = results
    assert hs == ds and hs["iterations"] > 3, (hs, ds)
    assert np.all(herr < 1e-7), herr
    for a, b in ((he, de), (herr, derr), (hx, dx), (hg, dg)):
        assert np.array_equal(dc.bits(a), dc.bits(b))
    # arrays of another context than the one given to use_context
    with pytest.raises(ValueError, match="use_context"):
        with sh.Context(0) as other:
            s = iterative_solver.LinearEigensystem(8, 1)
            try:
                s.solve(sh.DeviceRows(other, 1, 8), sh.DeviceRows(other, 1, 8), dev)
            finally:
                s.finalize()
