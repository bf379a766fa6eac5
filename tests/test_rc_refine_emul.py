"""The refined mode of the reverse-communication API (include/iterative_solver_c.h: Q_REFINE=1,
IterativeSolverHbmSetRefineAction) on the CPU, over the emulation of the f64 C ABI.  There the Q space is
stored in f64 (Q_STORAGE=f32 needs the mixed-precision ABI the emulation lacks, and is refused by name), so
nothing is rounded and delta = 0: what runs is the whole C-layer path -- option parsing and refusals, the
refine action called from inside AddVector on that call's own arrays, host and device routes -- with a root
declared converged only on the residual of its solution's own action.

The dense fixtures bh, hf, he with 1-3 roots at 1e-10, action x @ h in numpy; a child process, as
tests/test_device_api_emul.py."""
import os

import pytest

from test_device_api_emul import PRELUDE, needs_emul, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOLVES = PRELUDE + r"""
import rc_refine_cases as rc
from test_python_api_gpu import hamiltonian
ctx = sh.Context(0)
iterative_solver.use_context(ctx)
assert all(hasattr(iterative_solver._load(), n) for n in iterative_solver.REFINE_SIG)
THRESH = 1e-10
calls = 0
for name, split, roots in (("bh", 1e-8, (1, 2, 3)), ("hf", 1e-8, (1, 2, 3)), ("he", 0.0, (1,))):  # he: a degenerate pair
    h = hamiltonian(name, split)
    n = h.shape[0]
    d = np.diag(h).copy()
    recompute = n * rc.EPS * rc.norm2(h)  # the rounding of |H x - theta x| formed in f64
    for nroot in roots:
        guess = sorted(np.argsort(d, kind="stable")[:nroot])
        make = rc.eigen_solver(n, nroot, THRESH, "Q_REFINE=1")
        out = {}

        def loop(rec, out=out):
            x, g, nwork, act = rc.loop_refined(rec, nroot, n, lambda v: v @ h, d, guess)
            s = rec.s
            assert s.q_storage == 8
            r = rc.result(s, nroot, n, h, THRESH, nwork)
            out.setdefault("runs", []).append((r, act))
            return r["iterations"], act.sizes

        hl, dl, hr, dr = dc.both_routes(make, loop, ctx)
        dc.assert_same_log(hl, dl)
        assert hr == dr, (name, nroot, hr, dr)
        assert any(e[0] == "refine" for e in hl), (name, nroot)
        calls += len(hl)
        for r, act in out["runs"]:
            where = (name, nroot, r["errors"], r["residual_norms"])
            assert r["converged"], where
            # the action ran, never on more vectors than there are roots, never before the Q space existed
            assert len(act.sizes) >= 1 and max(act.sizes) <= nroot and min(act.q_creations) > 0, (where, act.sizes)
            st = r["refine"]
            assert st["refined_actions"] == sum(act.sizes) and st["first_refined_iteration"] >= 1, (where, st)
            assert st["max_delta"] == 0.0, st  # Q stored as R: nothing was rounded
            # the solver's errors ARE the residual norms of its solutions
            assert np.all(np.abs(r["errors"] - r["residual_norms"]) <= recompute), where
            assert np.all(r["residual_norms"] <= THRESH + recompute), where
print("calls compared:", calls)
print("ok")
"""

REFUSALS = PRELUDE + r"""
from test_python_api_gpu import hamiltonian
ctx = sh.Context(0)
iterative_solver.use_context(ctx)
h = hamiltonian("bh", 1e-8)
n = h.shape[0]


def refused(make, *words):
    before = int(iterative_solver._load().IterativeSolverHbmInstanceId())
    try:
        s = make()
    except RuntimeError as e:
        assert all(w.lower() in str(e).lower() for w in words), (words, str(e))
        assert int(iterative_solver._load().IterativeSolverHbmInstanceId()) == before  # nothing was pushed
    else:
        s.finalize()
        raise AssertionError(f"not refused: {words}")


eig = lambda options, hermitian=True, algorithm="": (lambda: iterative_solver.LinearEigensystem(
    n, 2, thresh=1e-10, hermitian=hermitian, algorithm=algorithm, options=options))
refused(eig("Q_STORAGE=f16"), "Q_STORAGE", "f16")
refused(eig("Q_STORAGE=f32"), "Q_STORAGE=f32", "mixed-precision")  # the emulation has no mixed ABI
refused(eig("Q_STORAGE=f32,Q_REFINE=1"), "Q_STORAGE=f32")
refused(eig("Q_REFINE=1", hermitian=False), "refine", "hermitian")
refused(eig("Q_REFINE=1,MAX_SIZE_QSPACE=12"), "refine", "max_size_qspace")
refused(eig("Q_REFINE=1,RESET_D=8"), "refine", "reset_D")
refused(eig("Q_REFINE=1,RESET_D_MAX_Q_SIZE=8"), "refine", "reset_D_max_Q_size")
refused(eig("Q_REFINE=1", algorithm="RSPT"), "Q_REFINE", "RSPT")
refused(eig("Q_STORAGE=f32", algorithm="RSPT"), "Q_STORAGE=f32", "RSPT")
refused(eig("Q_REFINE=1,Q_REFINE_KAPPA=-1"), "Q_REFINE_KAPPA")
rhs = np.ones((1, n))
for opt, word in (("Q_STORAGE=f32", "Q_STORAGE=f32"), ("Q_REFINE=1", "Q_REFINE")):
    refused(lambda: iterative_solver.LinearEquations(rhs, hermitian=True, options=opt), word, "LinearEquations")
    refused(lambda: iterative_solver.NonLinearEquations(n, options=opt), word, "NonLinearEquations")
    refused(lambda: iterative_solver.Optimize(n, options=opt), word, "Optimize")
# the defaults named explicitly are what no option is
for opt in ("Q_STORAGE=f64", "Q_REFINE=0", "q_storage = F64, q_refine = false"):
    s = eig(opt)()
    assert s.q_storage == 8 and s.refine_statistics() == {"refined_actions": 0, "first_refined_iteration": 0,
                                                           "max_delta": 0.0}
    assert s.quantise(np.full((2, n), 1 / 3)) == 0  # nothing to round
    s.finalize()

# a refinement that is needed while no action is set is an error naming the call that sets it
import rc_refine_cases as rc
d = np.diag(h).copy()
guess = sorted(np.argsort(d, kind="stable")[:2])
s = eig("Q_REFINE=1")()
try:
    rc.loop_refined(s, 2, n, lambda v: v @ h, d, guess, refine=False)
except RuntimeError as e:
    assert "IterativeSolverHbmSetRefineAction" in str(e), e
else:
    raise AssertionError("a refinement without an action did not raise")
s.finalize()
# ... and so it is after the action has been cleared again
s = eig("Q_REFINE=1")()
s.set_refine_action(lambda x, a: None)
s.set_refine_action(None)
try:
    rc.loop_refined(s, 2, n, lambda v: v @ h, d, guess, refine=False)
except RuntimeError as e:
    assert "IterativeSolverHbmSetRefineAction" in str(e), e
else:
    raise AssertionError("a refinement with a cleared action did not raise")
s.finalize()
# an exception inside the action reaches the caller of add_vector
s = eig("Q_REFINE=1")()


def boom(x, a):
    a[:, :] = x @ h
    raise KeyError("from the action")


s.set_refine_action(boom)
x, g = np.zeros((2, n)), np.zeros((2, n))
try:
    for k, i in enumerate(guess):
        x[k, i] = 1.0
    nwork = 2
    for _ in range(60):
        g[:nwork] = x[:nwork] @ h
        nwork = s.add_vector(x[:nwork], g[:nwork])
        ev = s.working_set_eigenvalues(nwork)
        for k in range(nwork):
            g[k] = g[k] / ((d - ev[k]) + 1e-15)
        nwork = s.end_iteration(x, g)
        assert nwork > 0, "converged without a refinement"
except KeyError as e:
    assert "from the action" in str(e)
else:
    raise AssertionError("the action's exception was lost")
s.finalize()
print("ok")
"""

SHARDED = PRELUDE + r"""
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
comm = sh.HubComm(rank, world, "127.0.0.1", int(os.environ["SSP_HUB_PORT"]))
ctx = sh.Context(0)
ctx.attach_host_comm(comm)
iterative_solver.use_context(ctx)
for opt, word in (("Q_REFINE=1", "Q_REFINE"), ("Q_STORAGE=f32", "Q_STORAGE=f32")):
    try:
        iterative_solver.LinearEigensystem(61, 2, hermitian=True, options=opt)
    except RuntimeError as e:
        assert word in str(e) and "rank" in str(e), e
    else:
        raise AssertionError("not refused on two ranks: " + opt)
s = iterative_solver.LinearEigensystem(61, 2, hermitian=True)  # without the options: as ever
s.finalize()
comm.barrier()
print("ok")
"""

PYTHON_SOLVE = PRELUDE + r"""
from test_python_api_gpu import hamiltonian
ctx = sh.Context(0)
iterative_solver.use_context(ctx)


class Dense(iterative_solver.Problem):
    def __init__(self, h):
        super().__init__()
        self.h, self.calls = h, []

    def action(self, parameters, actions):
        self.calls.append(parameters.shape[0])
        np.matmul(parameters, self.h, out=actions)

    def diagonals(self, d):
        d[:self.h.shape[0]] = np.diag(self.h)
        return True


h = hamiltonian("hf", 1e-8)
n, nroot = h.shape[0], 2
s = iterative_solver.LinearEigensystem(n, nroot, thresh=1e-10, hermitian=True, options="Q_REFINE=1")
x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
p = Dense(h)
s.solve(x, g, p, generate_initial_guess=True)
st = s.refine_statistics()
assert np.all(s.errors <= 1e-10) and st["refined_actions"] >= 1, (s.errors, st)
ev = s.eigenvalues.copy()
s.solution([0, 1], x, g)
for k in range(nroot):
    assert np.linalg.norm(x[k] @ h - ev[k] * x[k]) <= 1e-10 + n * np.finfo(float).eps * np.max(np.abs(np.linalg.eigvalsh(h)))
s.finalize()
print("ok")
"""


def check(r):
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


@needs_emul
def test_refined_solves_converge_on_true_residuals_and_both_routes_agree_bit_for_bit():
    check(run(SOLVES))


@needs_emul
def test_refusals_name_their_option_and_a_missing_action_names_its_call():
    check(run(REFUSALS))


@needs_emul
def test_either_option_is_refused_on_more_than_one_rank():
    import subprocess
    import sys

    from test_distributed import free_port

    port = free_port()
    procs = [subprocess.Popen([sys.executable, "-c", SHARDED, ROOT],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", SSP_HUB_PORT=str(port),
                                       OMP_NUM_THREADS="1"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]


@needs_emul
def test_python_solve_installs_the_problems_action():
    check(run(PYTHON_SOLVE))
