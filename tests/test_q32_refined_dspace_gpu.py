"""The refined f32 Q space under a Q-space limit (include/itsolv_hbm.h *_q32_refined_dspace; itsolv_hbm/solvers.h
set_refine_dspace) on the GPU: the consistent D space end to end.

1. dense n = 3000 at 1e-10 with the limit of tests/test_q32_refined_dspace_model.py (30, chosen there on the f64
   run alone), under refined_criteria of tests/test_q32_refined_gpu.py against the f64 solve with the same limit;
2. the short-vector path (fixture bh, n = 28), 2 roots at 1e-10, limit 4 nroots = 8;
3. synthetic n = 100003, 4 roots at 1e-8, max_p 0 and 8, limit 16, on the fused passes and call by call (child
   processes, SSP_FUSED_MIN_SIZE): the same iterations either way; fused, one combine_widen_f32 ledger call per
   rebuild and no gemm_outer_f32 from the rebuild;
4. the reverse-communication loop of tests/test_rc_refine_dspace_emul.py with Q_STORAGE=f32, host and device
   routes bit for bit;
5. a P space that is really rebuilt against: dense_3000 with max_p = 8 and the limit 30, on the fused passes and
   call by call (child processes), under refined_criteria with at least one rebuild.  This is what runs the P rows
   of update_dspace_refined (S(D,P), H(P,D) from [w, a].p) and the refined rows of new_qspace_data with nP != 0
   and nD != 0 together.  The issue's synthetic case with max_p = 8 does not: it converges before its Q space
   passes 16, and where a synthetic solve with a P space is made to rebuild (limit 12, or 1e-10) the Q vector
   that goes has coefficients near 1e-13 in every solution (the matrix has |H| near 1e5, so a correction of
   that size still moves the residual by 1e-8), below construct_dspace's norm_thresh of 1e-10: the projections
   are dropped as null, by the rule the f64 solver shares, the new D space is empty and the P rows never run.

Every reference is the f64 solve with the same limit; the bounds are refined_criteria's (true residuals within
threshold + n eps |H|_2, errors equal to them within that, eigenvalues within the sum of the residual norms,
iterations within +3).

Measured on an MI355X (profiles/r14/q32_refined_dspace.md).  dense_3000 with the limit 30: 41 iterations against
the f64 solve's 58, 10 rebuilds, 30 D-space actions, 66 refined actions.  bh: 17 against 16, 12 rebuilds; the
reverse-communication loop 18 against 15, 14 rebuilds; synthetic without a P space 6 against 6 with 1 rebuild,
with max_p = 8 6 against 6 and no rebuild (the solve ends before its Q space passes 16).  dense_3000 with
max_p = 8 (CPU model: 34 iterations against 46, 7 rebuilds, 21 D-space actions)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import device_api_cases as dc
import iterative_solver
import rc_refine_cases as rc
import rc_refine_dspace_cases as rd
from test_q32_refined_gpu import refined_criteria

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in cast")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "iterative-solver_amd")
EPS = float(np.finfo(np.float64).eps)
DENSE_LIMIT = 30  # tests/test_q32_refined_dspace_model.py LIMIT


def dspace_criteria(name, f64, ref, threshold, recompute, nroots):
    st = ref["refine_dspace"]
    print(f"\n{name}: D-space rebuilds {st['dspace_rebuilds']}, D-space actions {st['dspace_actions']}")
    assert st["dspace_rebuilds"] >= 1
    assert 1 <= st["dspace_actions"] <= nroots * st["dspace_rebuilds"]
    refined_criteria(name, f64, ref, threshold, recompute, nroots)


@pytest.fixture(scope="module")
def dense_3000():
    """tests/test_mixed_gpu.py dense_3000, and |H|_2."""
    n = 3000
    b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
    return h, float(np.max(np.abs(np.linalg.eigvalsh(h))))


def test_dense_3000_under_the_limit_reaches_1e_10(ctx, dense_3000):
    import itsolv_hbm as ih

    h, norm2 = dense_3000
    kw = dict(nroots=3, convergence_threshold=1e-10, max_iter=100, max_size_qspace=DENSE_LIMIT)
    f64 = ih.davidson_dense(ctx, h, **kw)
    ref = ih.davidson_dense(ctx, h, q32=True, refine=True, refine_dspace=True, **kw)
    assert ref["refine_dspace"]["dspace_rebuilds"] >= 5
    dspace_criteria(f"dense_3000 at 1e-10, limit {DENSE_LIMIT}", f64, ref, 1e-10, h.shape[0] * EPS * norm2, 3)


def test_short_vector_path_under_the_limit(ctx):
    """Fixture bh (n = 28: every vector on the short-vector path, the exact-mode combine_widen) with 2 roots."""
    import itsolv_hbm as ih
    from test_solver_gpu import hamiltonian

    h = hamiltonian("bh", 1e-8)
    kw = dict(nroots=2, convergence_threshold=1e-10, max_size_qspace=8)
    f64 = ih.davidson_dense(ctx, h, **kw)
    assert f64["converged"], "the f64 run must converge on bh at 1e-10 for this case to mean anything"
    ref = ih.davidson_dense(ctx, h, q32=True, refine=True, refine_dspace=True, **kw)
    norm2 = float(np.max(np.abs(np.linalg.eigvalsh((h + h.T) / 2))))
    dspace_criteria("bh at 1e-10, limit 8", f64, ref, 1e-10, h.shape[0] * EPS * norm2, 2)


def test_the_limit_without_the_opt_in_is_still_refused(ctx):
    import itsolv_hbm as ih

    h = np.diag(np.arange(1.0, 41.0)) + 0.01
    with pytest.raises(RuntimeError, match="max_size_qspace"):
        ih.davidson_dense(ctx, h, q32=True, refine=True, nroots=2, max_size_qspace=24)
    for kw in (dict(reset_D=8), dict(reset_D_max_Q_size=6)):
        with pytest.raises(RuntimeError, match="reset_D"):
            ih.davidson_dense(ctx, h, q32=True, refine=True, refine_dspace=True, nroots=2, max_size_qspace=24, **kw)
    with pytest.raises(ValueError, match="refine=True"):
        ih.davidson_dense(ctx, h, q32=True, refine_dspace=True, nroots=2, max_size_qspace=24)
    r = ih.davidson_dense(ctx, h, q32=True, refine=True, refine_dspace=True, nroots=2, max_size_qspace=6)
    assert r["converged"] and set(r["refine_dspace"]) == {"dspace_rebuilds", "dspace_actions"}


# ---- the bandwidth path, fused and call by call -------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import itsolv_hbm as ih
import subspace_hip as sh
max_p = int(sys.argv[2])
kw = dict(nroots=4, convergence_threshold=1e-8)
if max_p:
    kw["max_p"] = max_p
out = {}
with sh.Context(0) as ctx:
    for name, extra in (("f64", dict(max_size_qspace=16)),
                        ("dspace", dict(q32=True, refine=True, refine_dspace=True, max_size_qspace=16)),
                        ("refined", dict(q32=True, refine=True))):
        ctx.ledger_reset()
        ctx.ledger_enable(True)
        r = ih.davidson_synthetic(ctx, 100_003, 0.1, 2, 20251015, **dict(kw, **extra))
        ctx.synchronize()
        ctx.ledger_enable(False)
        calls = {}
        for op, v in ctx.ledger().items():
            op = op.split("(")[0].split(" [")[0]
            calls[op] = calls.get(op, 0) + v["calls"]
        out[name] = {"converged": bool(r["converged"]), "iterations": int(r["iterations"]),
                     "eigenvalues": [float(e) for e in r["eigenvalues"]], "errors": [float(e) for e in r["errors"]],
                     "residual_norms": [float(e) for e in r["residual_norms"]], "refine": r.get("refine"),
                     "refine_dspace": r.get("refine_dspace"), "calls": calls}
print(json.dumps(out))
"""


def solve(max_p, min_size):
    env = dict(os.environ, SSP_FUSED_MIN_SIZE=str(min_size))
    env.pop("SSP_ORTHO", None)
    env.pop("SSP_LEDGER_DETAIL", None)
    p = subprocess.run([sys.executable, "-c", CHILD, PKG, str(max_p)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    for r in out.values():
        for k in ("eigenvalues", "errors", "residual_norms"):
            r[k] = np.array(r[k])
    return out


@pytest.fixture(scope="module", params=[0, 8], ids=["no_p", "max_p8"])
def solves(request):
    """(fused, call by call) of one problem: each child runs the f64 solve with the limit, the refined solve with
    the limit and the consistent D space, and the refined solve without a limit; and max_p."""
    return solve(request.param, 0), solve(request.param, 10**15), request.param


def synth_criteria(name, run):
    f64, ref = run["f64"], run["dspace"]
    st = ref["refine_dspace"]
    print(f"\n{name}: iterations f64 {f64['iterations']} refined+dspace {ref['iterations']}, rebuilds "
          f"{st['dspace_rebuilds']}, D-space actions {st['dspace_actions']}, refined actions "
          f"{ref['refine']['refined_actions']}, max delta {ref['refine']['max_delta']:.3e}\n  errors {ref['errors']}\n"
          f"  residual norms {ref['residual_norms']}\n  f64 residual norms {f64['residual_norms']}")
    assert f64["converged"] and ref["converged"]
    # The solver's errors are true residuals in the refined mode, so they meet the threshold; residual_norms are
    # the runner's recomputation from the returned solutions.  Its worst-case rounding n eps |H|_2 is no use here
    # (|H|_2 is near 1e5 on this matrix: 2e-6), so the recomputation is asked to confirm the solver's figures
    # to the size of the threshold itself: each within 1e-8 of its error, hence below twice the threshold.
    assert np.all(ref["errors"] <= 1e-8)
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= 1e-8)
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= 2e-8)
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])
    assert ref["iterations"] <= f64["iterations"] + 3
    assert 0 <= st["dspace_actions"] <= 4 * st["dspace_rebuilds"]


def test_synthetic_under_the_limit_on_the_fused_passes(solves):
    synth_criteria("synthetic 100003 at 1e-8, limit 16, fused", solves[0])
    if solves[2] == 0:  # without a P space the 4 new vectors of every iteration pass the limit of 16 before the end
        assert solves[0]["dspace"]["refine_dspace"]["dspace_rebuilds"] >= 1
    ref, nolimit = solves[0]["dspace"], solves[0]["refined"]
    calls = ref["calls"]
    print(f"\nfused calls with the D space {calls}\nfused calls of the refined solve without a limit {nolimit['calls']}")
    # one pass per rebuild writes the new D parameters and their twins ...
    assert calls.get("combine_widen_f32", 0) == ref["refine_dspace"]["dspace_rebuilds"], calls
    # ... and the rebuild issues no gemm_outer_f32: the solve's gemm_outer_f32 rows are the dense passes of
    # construct_solution and of the block Gram-Schmidt update, one each per iteration whatever the subspace
    # holds (Q and D sources go concatenated), plus the extraction of the solutions at the end -- the count of
    # the refined solve without a limit, iteration for iteration
    assert calls["gemm_outer_f32"] - 2 * ref["iterations"] == nolimit["calls"]["gemm_outer_f32"] - 2 * nolimit["iterations"], \
        (calls, nolimit["calls"])
    assert nolimit["calls"].get("combine_widen_f32", 0) == 0 and nolimit["refine_dspace"] is None


def test_synthetic_under_the_limit_call_by_call(solves):
    synth_criteria("synthetic 100003 at 1e-8, limit 16, call by call", solves[1])
    assert solves[1]["dspace"]["calls"].get("combine_widen_f32", 0) == 0  # gemm_outer, then the widening copies
    assert solves[1]["dspace"]["iterations"] == solves[0]["dspace"]["iterations"]
    assert solves[1]["dspace"]["refine_dspace"] == solves[0]["dspace"]["refine_dspace"]


# ---- a P space that is rebuilt against: dense_3000 with max_p = 8, fused and call by call ----------------------
DENSE_P_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import itsolv_hbm as ih
import subspace_hip as sh
n = 3000
b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
h = (b + b.T) / 2
h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
kw = dict(nroots=3, convergence_threshold=1e-10, max_iter=100, max_size_qspace=int(sys.argv[2]), max_p=8)
out = {}
with sh.Context(0) as ctx:
    for name, extra in (("f64", {}), ("dspace", dict(q32=True, refine=True, refine_dspace=True))):
        r = ih.davidson_dense(ctx, h, **dict(kw, **extra))
        out[name] = {"converged": bool(r["converged"]), "iterations": int(r["iterations"]),
                     "eigenvalues": [float(e) for e in r["eigenvalues"]], "errors": [float(e) for e in r["errors"]],
                     "residual_norms": [float(e) for e in r["residual_norms"]], "refine": r.get("refine"),
                     "refine_dspace": r.get("refine_dspace")}
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def dense_p_solves():
    """(fused, call by call): the f64 solve and the refined solve with the consistent D space, both with a P space
    of 8 unit vectors and the limit of the dense case."""
    runs = []
    for min_size in (0, 10**15):
        env = dict(os.environ, SSP_FUSED_MIN_SIZE=str(min_size))
        env.pop("SSP_ORTHO", None)
        p = subprocess.run([sys.executable, "-c", DENSE_P_CHILD, PKG, str(DENSE_LIMIT)], capture_output=True, text=True,
                           timeout=300, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        out = json.loads(p.stdout.strip().splitlines()[-1])
        for r in out.values():
            for k in ("eigenvalues", "errors", "residual_norms"):
                r[k] = np.array(r[k])
        runs.append(out)
    return runs


@pytest.mark.parametrize("which", [0, 1], ids=["fused", "call_by_call"])
def test_dense_3000_with_a_p_space_rebuilds_under_the_limit(dense_p_solves, dense_3000, which):
    """The P rows of the rebuilt D blocks and the refined rows with nP != 0 and nD != 0 together."""
    h, norm2 = dense_3000
    run = dense_p_solves[which]
    dspace_criteria(f"dense_3000 with max_p = 8 at 1e-10, limit {DENSE_LIMIT}, {('fused', 'call by call')[which]}",
                    run["f64"], run["dspace"], 1e-10, h.shape[0] * EPS * norm2, 3)
    assert run["dspace"]["refine_dspace"]["dspace_rebuilds"] >= 1
    assert run["dspace"]["refine_dspace"]["dspace_actions"] >= 1  # a D space that is not empty, against a P space


def test_dense_3000_with_a_p_space_fused_and_call_by_call_agree(dense_p_solves):
    fused, calls = (r["dspace"] for r in dense_p_solves)
    assert fused["iterations"] == calls["iterations"] and fused["refine_dspace"] == calls["refine_dspace"]


# ---- the reverse-communication loop over an f32 Q space ------------------------------------------------------
@pytest.fixture()
def api(ctx):
    iterative_solver.use_context(ctx)
    yield ctx
    iterative_solver.use_context(None)


def test_rc_loop_with_an_f32_q_space_host_and_device_routes(api):
    from test_python_api_gpu import hamiltonian

    h = hamiltonian("bh", 1e-8)
    n, nroot, limit, thresh = h.shape[0], 2, 8, 1e-10
    d = np.diag(h).copy()
    guess = sorted(np.argsort(d, kind="stable")[:nroot])
    apply = lambda v: v @ h  # noqa: E731
    recompute = n * EPS * rc.norm2(h)
    s = rc.eigen_solver(n, nroot, thresh, f"MAX_SIZE_QSPACE={limit}")()
    f64 = rc.result(s, nroot, n, h, thresh, rd.plain_loop(s, nroot, n, apply, d, guess))
    s.finalize()
    make = rc.eigen_solver(n, nroot, thresh, f"Q_STORAGE=f32,Q_REFINE=1,Q_REFINE_DSPACE=1,MAX_SIZE_QSPACE={limit}")
    out = []

    def loop(rec):
        assert rec.s.q_storage == 4
        x, g, nwork, act, inside = rd.loop(rec, nroot, n, apply, rc.stored(d), guess)
        r = rc.result(rec.s, nroot, n, h, thresh, nwork)
        r["refine_dspace"] = rec.s.refine_dspace_statistics
        out.append((r, act, inside))
        return r["iterations"], act.sizes, inside

    hl, dl, hr, dr = dc.both_routes(make, loop, api)
    dc.assert_same_log(hl, dl)
    assert hr == dr, (hr, dr)
    for r, act, inside in out:
        st = r["refine_dspace"]
        assert len(inside) == st["dspace_rebuilds"] and sum(inside) == st["dspace_actions"] and max(inside) <= nroot
        assert r["refine"]["refined_actions"] == sum(act.sizes) - sum(inside) and r["refine"]["max_delta"] > 0
        dspace_criteria("RC bh at 1e-10, limit 8, Q_STORAGE=f32", f64, r, thresh, recompute, nroot)
