"""The f32 Q space behind the reverse-communication API (include/iterative_solver_c.h: Q_STORAGE=f32, Q_REFINE=1,
IterativeSolverHbmSetRefineAction) on the GPU, on the session context.

Plain mode (Q_STORAGE=f32): host and device routes bit for bit, call by call (tests/device_api_cases.py), on the
short-vector path, the bandwidth path and the fused passes; the instance really runs the mixed kernels and holds
its Q vectors in half the bytes; against the f64 instance the assertions of
tests/test_mixed_gpu.py::test_davidson_with_f32_q_space_matches_the_f64_run.

Refined mode (Q_STORAGE=f32,Q_REFINE=1): refined_criteria of tests/test_q32_refined_gpu.py with the f64 side
the same loop on an f64 instance; the stall without Q_REFINE; host and device routes bit for bit through the
refinements; the device route rounds in its export (no quantise pass), the host route in a pass of its own;
the statistics; quantise(); and the Python solve() drivers."""
import numpy as np
import pytest

import device_api_cases as dc
import iterative_solver
import rc_refine_cases as rc
import subspace_hip as sh
from test_device_api_gpu import synthetic
from test_python_api_gpu import hamiltonian
from test_q32_refined_gpu import refined_criteria

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in cast")]
EPS, EPS32 = rc.EPS, float(np.finfo(np.float32).eps)
F32, F64 = np.float32, np.float64
PLAIN, REFINED = "Q_STORAGE=f32", "Q_STORAGE=f32,Q_REFINE=1"


@pytest.fixture()
def api(ctx):
    iterative_solver.use_context(ctx)
    yield ctx
    iterative_solver.use_context(None)


@pytest.fixture(scope="module")
def dense_3000():
    """tests/test_mixed_gpu.py dense_3000, and |H|_2."""
    n = 3000
    b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
    return h, float(np.max(np.abs(np.linalg.eigvalsh(h))))


def calls(led, name):
    return sum(v["calls"] for op, v in led.items() if op.split("(")[0].split(" [")[0] == name)


def route(make, loop, ctx, device, ld=None):
    """One route of device_api_cases.both_routes, with the context's ledger of it: (log, result, ledger)."""
    log = []
    solver = make()
    target = dc.ViaDevice(solver, ctx, ld) if device else solver
    ctx.ledger_reset()
    ctx.ledger_enable(True)
    try:
        res = loop(dc.Recorded(target, solver, log))
        ctx.synchronize()
        led = ctx.ledger()
    finally:
        ctx.ledger_enable(False)
        solver.finalize()
    return log, res, led


# ---- plain mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [None, 29], ids=["aligned", "alternating"])
def test_plain_routes_agree_on_the_short_vector_path(api, ld):
    h = hamiltonian("bh", 1e-8)
    n, nroot = h.shape[0], 2
    d = np.diag(h).copy()
    guess = sorted(np.argsort(d, kind="stable")[:nroot])
    make = rc.eigen_solver(n, nroot, 1e-6, PLAIN)
    loop = lambda s: dc.loop_davidson(s, nroot, n, lambda x: x @ h, rc.stored(d), guess)  # noqa: E731
    hl, dl, _, _ = dc.both_routes(make, loop, api, ld=ld)
    dc.assert_same_log(hl, dl)
    assert hl[-1][0] == "solution" and np.all(hl[-1][2] <= 1e-6) and len(hl) > 6


@pytest.mark.parametrize("n,nroot,ld,max_iter", [(100_003, 4, None, 40), (2**20 + 5, 2, 2**20 + 5, 6),
                                                 (2**20 + 5, 2, 2**20 + 6, 6)],
                         ids=["100003", "2^20+5-ld=n", "2^20+5-ld=n+1"])
def test_plain_routes_agree_on_the_synthetic_problem(api, n, nroot, ld, max_iter):
    """n = 100003 to convergence at the plain mode's 1e-6; n = 2^20 + 5: the fused passes, 6 iterations."""
    action, diag, release = synthetic(api, n)
    make = rc.eigen_solver(n, nroot, 1e-6, PLAIN)
    loop = lambda s: dc.loop_davidson(s, nroot, n, action, rc.stored(diag), list(range(nroot)),  # noqa: E731
                                      max_iter=max_iter)
    hlog, _, hled = route(make, loop, api, False)
    dlog, _, dled = route(make, loop, api, True, ld)
    release()
    dc.assert_same_log(hlog, dlog)
    assert hlog[-1][0] == "solution" and len(hlog) >= min(2 * max_iter, 9)
    if max_iter > 6:
        assert np.all(hlog[-1][2] <= 1e-6), hlog[-1][2]
    for led in (hled, dled):  # the instance runs on the f32 Q space's kernels
        assert calls(led, "gemm_outer_f32") > 0, sorted(led)
        assert calls(led, "gemm_inner_cols") + calls(led, "gemm_inner_f32") > 0, sorted(led)
    assert calls(dled, "rows_export_q") == 0 and calls(dled, "quantise_f32") == 0  # nothing is rounded in plain mode


def block(nbytes):
    """The arena's block for a request: below 1 MiB rounded to 256 B, else to 2 MiB."""
    return (nbytes + 255) // 256 * 256 if nbytes < 2**20 else (nbytes + 2**21 - 1) // 2**21 * 2**21


@pytest.mark.parametrize("n", [100_003, 2**20 + 5])
def test_plain_instance_reports_its_storage_and_holds_q_in_half_the_bytes(api, n):
    nroot, iters = 2, 3
    action, diag, release = synthetic(api, n)
    in_use, stored = {}, {}
    for options in ("", PLAIN):
        s = rc.eigen_solver(n, nroot, 1e-6, options)()
        d = rc.stored(diag) if options else diag
        assert s.q_storage == (4 if options else 8)
        assert int(iterative_solver._load().IterativeSolverHbmQStorage()) == s.q_storage
        x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
        x[np.arange(nroot), np.arange(nroot)] = 1.0
        for _ in range(iters):  # full working sets: every add_vector stores nroot parameter and action vectors
            g[:] = action(x)
            assert s.add_vector(x, g) == nroot
            ev = s.working_set_eigenvalues(nroot)
            for k in range(nroot):
                g[k] = g[k] / ((d - ev[k]) + 1e-15)
            assert s.end_iteration(x, g) == nroot
        # the end of a reverse-communication loop, as device_api_cases.loop_davidson ends: every staging vector has
        # just been written in full, so none shares its block with another (hbm::Vec copies share until written)
        s.solution(list(range(nroot)), x, g)
        api.synchronize()
        in_use[options], stored[options] = api.memory_stats()[0], s.statistics()["q_creations"]
        s.finalize()
    release()
    assert stored[""] == stored[PLAIN] == 2 * nroot * iters
    print(f"\nn = {n}: bytes in use f64 {in_use['']}, f32 {in_use[PLAIN]}, stored Q vectors {stored[PLAIN]}")
    assert in_use[""] - in_use[PLAIN] == stored[PLAIN] * (block(8 * n) - block(4 * n))


def dense_run(h, nroot, threshold, options, refine, max_iter=60):
    n = h.shape[0]
    d = np.diag(h).copy()
    guess = sorted(np.argsort(d, kind="stable")[:nroot])
    s = rc.eigen_solver(n, nroot, threshold, options)()
    if s.q_storage == 4:
        d = rc.stored(d)
    try:
        _, _, nwork, act = rc.loop_refined(s, nroot, n, lambda x: x @ h, d, guess, max_iter=max_iter, refine=refine)
        return rc.result(s, nroot, n, h, threshold, nwork), act
    finally:
        s.finalize()


def test_plain_against_the_f64_instance_on_dense_3000(api, dense_3000):
    h, norm2 = dense_3000
    f64, _ = dense_run(h, 3, 1e-6, "", False)
    q32, _ = dense_run(h, 3, 1e-6, PLAIN, False)
    bound = 4 * EPS32 * norm2
    diff = np.max(np.abs(q32["eigenvalues"] - f64["eigenvalues"]))
    print(f"\nRC q32 n=3000: iterations f64 {f64['iterations']} q32 {q32['iterations']}, max |theta_q32 - theta_f64| "
          f"{diff:.3e} (bound {bound:.3e}), q32 residual norms {q32['residual_norms']}")
    assert f64["converged"] and q32["converged"]
    assert diff <= bound
    assert np.all(q32["residual_norms"] <= 1e-6 + bound)
    assert q32["iterations"] <= f64["iterations"] + 3


# ---- refined mode -------------------------------------------------------------------------------------------
def test_refined_dense_3000_reaches_1e_10_and_plain_does_not(api, dense_3000):
    h, norm2 = dense_3000
    f64, _ = dense_run(h, 3, 1e-10, "", False)
    ref, act = dense_run(h, 3, 1e-10, REFINED, True)
    refined_criteria("RC dense_3000 at 1e-10", f64, ref, 1e-10, h.shape[0] * EPS * norm2, 3)
    st = ref["refine"]
    assert st["refined_actions"] == sum(act.sizes) and max(act.sizes) <= 3 and st["max_delta"] > 0, (st, act.sizes)
    plain, _ = dense_run(h, 3, 1e-10, PLAIN, False)
    print(f"\nRC plain q32 at 1e-10: iterations {plain['iterations']}, errors {plain['errors']}")
    assert not plain["converged"]


def test_refined_short_vector_path(api):
    h = hamiltonian("bh", 1e-8)
    f64, _ = dense_run(h, 2, 1e-10, "", False)
    assert f64["converged"], "the f64 run must converge on bh at 1e-10 for this case to mean anything"
    ref, act = dense_run(h, 2, 1e-10, REFINED, True)
    refined_criteria("RC bh at 1e-10", f64, ref, 1e-10, h.shape[0] * EPS * rc.norm2(h), 2)
    assert ref["refine"]["refined_actions"] == sum(act.sizes)


def refined_routes(api, n, nroot, threshold, apply, diag, guess, ld=None):
    make = rc.eigen_solver(n, nroot, threshold, REFINED)
    acts = []

    def loop(rec):
        x, g, nwork, act = rc.loop_refined(rec, nroot, n, apply, rc.stored(diag), guess)
        acts.append((act, rec.s.refine_statistics(), rec.s.errors.copy(), nwork))
        return nwork

    hlog, _, hled = route(make, loop, api, False)
    dlog, _, dled = route(make, loop, api, True, ld)
    dc.assert_same_log(hlog, dlog)
    assert any(e[0] == "refine" for e in hlog)
    for act, st, errors, nwork in acts:
        assert nwork == 0 and np.all(errors <= threshold), errors
        assert st["refined_actions"] == sum(act.sizes) and max(act.sizes) <= nroot and min(act.q_creations) > 0
    ends = sum(1 for e in hlog if e[0] == "end_iteration" and e[1] > 0)
    # the device route rounds in its export, the host route in a pass over the staging vectors
    assert calls(dled, "quantise_f32") == 0 and calls(dled, "rows_export_q") == ends, (ends, sorted(dled))
    assert calls(hled, "quantise_f32") == ends and calls(hled, "rows_export_q") == 0, (ends, sorted(hled))
    return hlog


@pytest.mark.parametrize("ld", [None, 29], ids=["aligned", "alternating"])
def test_refined_routes_agree_on_the_short_vector_path(api, ld):
    h = hamiltonian("bh", 1e-8)
    n, nroot = h.shape[0], 2
    d = np.diag(h).copy()
    refined_routes(api, n, nroot, 1e-10, lambda x: x @ h, d, sorted(np.argsort(d, kind="stable")[:nroot]), ld)


def test_refined_routes_agree_on_the_synthetic_problem(api):
    n, nroot = 100_003, 4
    action, diag, release = synthetic(api, n)
    try:
        refined_routes(api, n, nroot, 1e-8, action, diag, list(range(nroot)))
    finally:
        release()


def test_quantise_rounds_a_guess_as_numpy_does(api):
    n = 4099
    r = np.random.default_rng(3)
    x = r.uniform(-2, 2, (3, n)) * 10.0 ** r.integers(-3, 4, (3, n))
    want = x.astype(F32).astype(F64)
    assert not np.array_equal(want, x)
    s = rc.eigen_solver(n, 3, 1e-8, REFINED)()
    try:
        host = x.copy()
        assert s.quantise(host) == 3
        assert np.array_equal(dc.bits(host), dc.bits(want))
        buf = api.alloc(3 * n)
        for rows in (sh.DeviceRows(api, 3, n), sh.DeviceRows(api, 3, n, n, ptr=buf.ptr)):  # aligned; alternating parity
            rows.upload(x)
            assert s.quantise(rows) == 3
            assert np.array_equal(dc.bits(rows.numpy()), dc.bits(want)), rows.ld
        one = api.upload(x[0])
        assert s.quantise(one) == 1 and np.array_equal(dc.bits(one.numpy()), dc.bits(want[0]))
    finally:
        s.finalize()


class Dense(iterative_solver.Problem):
    """H as a numpy matrix; on device arrays the same numpy work on downloaded rows."""

    def __init__(self, h):
        super().__init__()
        self.h = h

    def action(self, parameters, actions):
        if isinstance(parameters, np.ndarray):
            np.matmul(parameters, self.h, out=actions)
        else:
            actions.upload(parameters.numpy() @ self.h)

    def diagonals(self, d):
        if isinstance(d, np.ndarray):
            d[:self.h.shape[0]] = np.diag(self.h)
        else:
            d.ctx.upload_into(d, np.diag(self.h).copy())
        return True

    def precondition(self, residual, shift=None, diagonals=None):
        if not isinstance(residual, np.ndarray):
            return super().precondition(residual, shift, diagonals)
        for k in range(residual.shape[0]):
            residual[k] = residual[k] / ((diagonals - shift[k]) + 1e-15)


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device_rows"])
def test_python_solve_in_refined_mode(api, dense_3000, device):
    h, norm2 = dense_3000
    n, nroot = h.shape[0], 3
    f64, _ = dense_run(h, nroot, 1e-10, "", False)
    s = rc.eigen_solver(n, nroot, 1e-10, REFINED)()
    try:
        if device:
            x, g = sh.DeviceRows(api, nroot, n), sh.DeviceRows(api, nroot, n)
        else:
            x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
        s.solve(x, g, Dense(h), generate_initial_guess=True, max_iter=60)
        ref = rc.result(s, nroot, n, h, 1e-10, 0 if np.all(s.errors <= 1e-10) else nroot)
    finally:
        s.finalize()
    refined_criteria(f"solve() dense_3000 at 1e-10, device={device}", f64, ref, 1e-10, n * EPS * norm2, nroot)
