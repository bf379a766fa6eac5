"""The refined mode of the reverse-communication API under a Q-space limit (include/iterative_solver_c.h:
Q_REFINE=1, Q_REFINE_DSPACE=1, MAX_SIZE_QSPACE) on the CPU, over the emulation of the f64 C ABI.  There the Q
space is stored in f64, so nothing is rounded and delta = 0: what runs is the whole C-layer path -- option
parsing and refusals, the D-space rebuild inside EndIteration / EndIterationDevice with the refine action called
on that call's own arrays, host and device routes bit for bit, the statistics -- and the solver's consistent
D space (true actions, D blocks from the twins) through the generic handler paths.

The reference is the plain f64 loop with the same MAX_SIZE_QSPACE.  The bound on the eigenvalues is the sum of
the two solves' true residual norms (each Ritz value is within its residual norm of an eigenvalue, and the
roots are separated by far more than 1e-10); the iteration margin is the project's +3.  The limits are 4 nroot
(2 nroot is the chaotic regime of the reference algorithm), on the fixture bh (n = 28),
where the plain loop rebuilds its D space 11 and 9 times."""
import os
import subprocess
import sys

from test_device_api_emul import PRELUDE, needs_emul, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOLVES = PRELUDE + r"""
import rc_refine_cases as rc
import rc_refine_dspace_cases as rd
from test_python_api_gpu import hamiltonian
ctx = sh.Context(0)
iterative_solver.use_context(ctx)
assert all(hasattr(iterative_solver._load(), n) for n in iterative_solver.DSPACE_SIG)
THRESH = 1e-10
h = hamiltonian("bh", 1e-8)
n = h.shape[0]
d = np.diag(h).copy()
recompute = n * rc.EPS * rc.norm2(h)
apply = lambda v: v @ h
for nroot in (2, 3):
    limit = 4 * nroot
    guess = sorted(np.argsort(d, kind="stable")[:nroot])
    s = rc.eigen_solver(n, nroot, THRESH, f"MAX_SIZE_QSPACE={limit}")()
    plain = rc.result(s, nroot, n, h, THRESH, rd.plain_loop(s, nroot, n, apply, d, guess))
    s.finalize()
    assert plain["converged"], plain["errors"]
    make = rc.eigen_solver(n, nroot, THRESH, f"Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE={limit}")
    out = []

    def loop(rec):
        x, g, nwork, act, inside = rd.loop(rec, nroot, n, apply, d, guess)
        r = rc.result(rec.s, nroot, n, h, THRESH, nwork)
        r["dspace"] = rec.s.refine_dspace_statistics
        out.append((r, act, inside))
        return r["iterations"], act.sizes, inside

    hl, dl, hr, dr = dc.both_routes(make, loop, ctx)
    dc.assert_same_log(hl, dl)
    assert hr == dr, (nroot, hr, dr)
    for r, act, inside in out:
        where = (nroot, r["iterations"], plain["iterations"], r["dspace"], r["errors"])
        print("bh", nroot, "limit", limit, "iterations", r["iterations"], "plain", plain["iterations"], r["dspace"], r["refine"])
        assert r["converged"], where
        assert r["iterations"] <= plain["iterations"] + 3, where
        assert np.all(np.abs(r["eigenvalues"] - plain["eigenvalues"]) <= r["residual_norms"] + plain["residual_norms"]), where
        assert np.all(r["residual_norms"] <= THRESH + recompute), where
        assert np.all(np.abs(r["errors"] - r["residual_norms"]) <= recompute), where
        # the refine action was called from inside end_iteration, once per rebuild, never on more than nroot rows
        st = r["dspace"]
        assert st["dspace_rebuilds"] >= 1 and st["dspace_actions"] > 0, where
        assert len(inside) == st["dspace_rebuilds"] and sum(inside) == st["dspace_actions"], (where, inside)
        assert max(inside) <= nroot and st["dspace_actions"] <= nroot * st["dspace_rebuilds"], (where, inside)
        # ... and the refined residuals' actions are counted apart from them
        assert r["refine"]["refined_actions"] == sum(act.sizes) - sum(inside), (where, act.sizes)
        assert r["refine"]["max_delta"] == 0.0  # Q stored as R: nothing was rounded
print("ok")
"""

# Q_REFINE_DSPACE_SLACK: how far below the limit a rebuild cuts the Q space.  At limit = 4 nroot the solver's rule
# gives 0 (a rebuild in every iteration once the Q space is full), so SLACK=0 is the same solve; one working set
# (nroot) leaves room for one iteration without a rebuild after each, so there are fewer rebuilds per iteration.
SLACK = PRELUDE + r"""
import rc_refine_cases as rc
import rc_refine_dspace_cases as rd
from test_python_api_gpu import hamiltonian
ctx = sh.Context(0)
iterative_solver.use_context(ctx)
THRESH, nroot = 1e-10, 3
limit = 4 * nroot
h = hamiltonian("bh", 1e-8)
n = h.shape[0]
d = np.diag(h).copy()
guess = sorted(np.argsort(d, kind="stable")[:nroot])
apply = lambda v: v @ h
s = rc.eigen_solver(n, nroot, THRESH, f"MAX_SIZE_QSPACE={limit}")()
plain = rc.result(s, nroot, n, h, THRESH, rd.plain_loop(s, nroot, n, apply, d, guess))
s.finalize()
got = {}
for name, extra in (("rule", ""), ("0", ",Q_REFINE_DSPACE_SLACK=0"), ("nroot", f",Q_REFINE_DSPACE_SLACK={nroot}"),
                    ("huge", ",Q_REFINE_DSPACE_SLACK=1000")):
    s = rc.eigen_solver(n, nroot, THRESH, f"Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE={limit}" + extra)()
    x, g, nwork, act, inside = rd.loop(s, nroot, n, apply, d, guess)
    r = rc.result(s, nroot, n, h, THRESH, nwork)
    r["dspace"] = s.refine_dspace_statistics
    s.finalize()
    print("slack", name, "iterations", r["iterations"], r["dspace"], "plain", plain["iterations"])
    assert r["converged"], (name, r["errors"])
    assert np.all(np.abs(r["eigenvalues"] - plain["eigenvalues"]) <= r["residual_norms"] + plain["residual_norms"]), name
    assert r["dspace"]["dspace_rebuilds"] >= 1 and len(inside) == r["dspace"]["dspace_rebuilds"], (name, inside)
    got[name] = r
assert got["0"]["iterations"] == got["rule"]["iterations"] and got["0"]["dspace"] == got["rule"]["dspace"]
assert np.array_equal(got["0"]["eigenvalues"], got["rule"]["eigenvalues"])
per_iteration = lambda r: r["dspace"]["dspace_rebuilds"] / r["iterations"]
assert per_iteration(got["nroot"]) < per_iteration(got["0"]), (got["nroot"]["dspace"], got["0"]["dspace"])
# a value beyond the limit is cut so that nroot Q vectors stay
assert got["huge"]["converged"]
print("ok")
"""

REFUSALS = PRELUDE + r"""
from test_python_api_gpu import hamiltonian
import rc_refine_cases as rc
import rc_refine_dspace_cases as rd
ctx = sh.Context(0)
iterative_solver.use_context(ctx)
h = hamiltonian("bh", 1e-8)
n = h.shape[0]


def refused(options, *words):
    before = int(iterative_solver._load().IterativeSolverHbmInstanceId())
    try:
        s = iterative_solver.LinearEigensystem(n, 2, thresh=1e-10, hermitian=True, options=options)
    except RuntimeError as e:
        assert all(w.lower() in str(e).lower() for w in words), (words, str(e))
        assert int(iterative_solver._load().IterativeSolverHbmInstanceId()) == before  # nothing was pushed
    else:
        s.finalize()
        raise AssertionError(f"not refused: {options}")


refused("Q_REFINE_DSPACE=1", "Q_REFINE_DSPACE", "Q_REFINE=1")
refused("Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE=8", "Q_REFINE_DSPACE", "Q_REFINE=1")
refused("Q_REFINE=0,Q_REFINE_DSPACE=1", "Q_REFINE_DSPACE", "Q_REFINE=1")
refused("Q_REFINE=1,Q_REFINE_DSPACE_SLACK=2", "Q_REFINE_DSPACE_SLACK", "Q_REFINE_DSPACE=1")
refused("Q_REFINE=1,Q_REFINE_DSPACE=1,Q_REFINE_DSPACE_SLACK=-1,MAX_SIZE_QSPACE=8", "Q_REFINE_DSPACE_SLACK", "negative")
refused("Q_REFINE=1,Q_REFINE_DSPACE=1,RESET_D=8", "refine", "reset_D")
refused("Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE=8,RESET_D=8", "refine", "reset_D")
refused("Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE=8,RESET_D_MAX_Q_SIZE=6", "refine", "reset_D_max_Q_size")
refused("Q_REFINE=1,Q_REFINE_DSPACE=0,MAX_SIZE_QSPACE=8", "refine", "max_size_qspace")  # the opt-in off: as ever
refused("Q_REFINE=1,MAX_SIZE_QSPACE=8", "refine", "max_size_qspace")
# accepted: with the limit, and without one (then nothing is ever rebuilt)
for opt in ("Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE=8", "Q_REFINE=1,Q_REFINE_DSPACE=1"):
    s = iterative_solver.LinearEigensystem(n, 2, thresh=1e-10, hermitian=True, options=opt)
    assert s.refine_dspace_statistics == {"dspace_rebuilds": 0, "dspace_actions": 0}
    s.finalize()
# a rebuild that is needed while no action is set is an error naming the call that sets it
d = np.diag(h).copy()
guess = sorted(np.argsort(d, kind="stable")[:2])
s = iterative_solver.LinearEigensystem(n, 2, thresh=1e-10, hermitian=True, options="Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE=4")
try:
    rd.plain_loop(s, 2, n, lambda v: v @ h, d, guess)
except RuntimeError as e:
    assert "IterativeSolverHbmSetRefineAction" in str(e), e
else:
    raise AssertionError("a rebuild without an action did not raise")
s.finalize()
print("ok")
"""

SHARDED = PRELUDE + r"""
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
comm = sh.HubComm(rank, world, "127.0.0.1", int(os.environ["SSP_HUB_PORT"]))
ctx = sh.Context(0)
ctx.attach_host_comm(comm)
iterative_solver.use_context(ctx)
try:
    iterative_solver.LinearEigensystem(61, 2, hermitian=True, options="Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE=8")
except RuntimeError as e:
    assert "Q_REFINE_DSPACE" in str(e) and "rank" in str(e), e  # the refusal names the option that was asked for
else:
    raise AssertionError("not refused on two ranks")
comm.barrier()
print("ok")
"""


def check(r):
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


@needs_emul
def test_rc_loop_under_a_q_limit_converges_and_rebuilds_inside_end_iteration():
    check(run(SOLVES))


@needs_emul
def test_the_slack_option_sets_the_rebuild_schedule():
    check(run(SLACK))


@needs_emul
def test_the_option_needs_q_refine_and_the_resets_stay_refused():
    check(run(REFUSALS))


@needs_emul
def test_the_option_is_refused_on_two_ranks():
    from test_distributed import free_port

    port = free_port()
    procs = [subprocess.Popen([sys.executable, "-c", SHARDED, ROOT],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", SSP_HUB_PORT=str(port),
                                       OMP_NUM_THREADS="1"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0 and out.strip().endswith("ok"), out[-4000:]
