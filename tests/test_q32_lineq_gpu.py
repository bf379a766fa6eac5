"""Linear equations with the Q space in f32, plain and refined (include/subspace_hip.h ssp_mx_rhs_residual_norms;
include/itsolv_hbm.h itsolv_linear_equations_*; Q_STORAGE=f32[,Q_REFINE=1] of IterativeSolverLinearEquationsInitialize).

1. the kernel: yy bit for bit numpy's (ys * y - float64(b)) * s and the unfused sequence on the same context, the
   norms within the reduction bar of numpy's sum and, on the short-vector path, bit for bit the sequence's dots;
   repeat calls, the ledger row, pending zero fills, n = 0, argument errors;
2. dense n = 3000 at 1e-10: f64, refined and plain with the criteria of tests/test_q32_lineq_model.py, and the refined
   solve again with max_p = 8;
3. dense at 1e-6 in plain q32;
4. synthetic n = 100003 (rank 4, 3 right-hand sides, 1e-8) refined, on the fused passes and call by call (child
   processes, SSP_FUSED_MIN_SIZE), against the f64 synthetic entry, with the ledgers;
5. the short-vector path (fixture bh, shifted to be positive definite);
6. the reverse-communication API through the host and the device routes;
7. the refusals, each naming its option.

Bounds.  recompute_r = n eps (|A|_2 |x_r| + |b_r|) / |b_r| is the worst-case rounding of a relative residual
recomputed in f64 from x_r.  For positive definite A two solutions of one system differ by at most
(res_a + res_b) |b| / lambda_min(A).  A plain f32 Q space of k vectors stores the right-hand side and every
action rounded: the solver's estimate is off its true residual by at most 2^-24 (|A|_2 sqrt(k) |x_r| + |b_r|) / |b_r|."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in cast")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "iterative-solver_amd")
EPS = float(np.finfo(np.float64).eps)
U32 = 2.0**-24
F32, F64 = np.float32, np.float64
EXACT_MAX_DEFAULT = 2048  # ssp_ctx_set_exact_max default (include/subspace_hip.h)
K_OUTER_DST = 16  # vectors per launch

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, (1 << 20) + 5]
COUNTS = [1, 2, 3, 4, 5, 8, 16, 17]
SCALES = [1.0, 0.3, -(2.0**-30)]


def test_the_lengths_are_those_of_the_refined_kernel_tests():
    from test_q32_refined_gpu import LENGTHS as theirs

    assert LENGTHS == theirs


def bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


@pytest.fixture
def exact_max(ctx, request):
    ctx.set_exact_max(request.param)
    yield request.param
    ctx.set_exact_max(EXACT_MAX_DEFAULT)


def ledger_of(ctx, f):
    ctx.ledger_reset()
    ctx.ledger_enable(True)
    try:
        r = f()
        ctx.synchronize()
        return r, ctx.ledger()
    finally:
        ctx.ledger_enable(False)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("exact_max", [EXACT_MAX_DEFAULT, 0], indirect=True, ids=["exact_default", "exact_0"])
def test_kernel_is_the_unfused_sequence_bit_for_bit(ctx, exact_max, n):
    rng = np.random.default_rng(n)
    mmax = max(COUNTS)
    y_host = [rng.uniform(-2, 2, n) * 10.0 ** rng.integers(-3, 4, n) for _ in range(mmax)]
    b_host = {F64: [rng.uniform(-2, 2, n) * 10.0 ** rng.integers(-3, 4, n) for _ in range(mmax)]}
    b_host[F32] = [b.astype(F32) for b in b_host[F64]]
    y0 = [ctx.upload(v) for v in y_host]  # pristine copies: every run starts from a device copy of these
    yy = [ctx.alloc(n) for _ in range(mmax)]
    exact = 0 < n <= exact_max
    for tb in (F32, F64):
        bb = [ctx.upload(b, tb) for b in b_host[tb]]
        for m in COUNTS:
            # (s_j, ys_j) over the vectors of a call: every scale beside a different one, no pending scale at all,
            # and (short vectors only: the same kernels, fewer bytes to check) every scale beside itself
            variants = [(0, 1), (1, None)] + ([(0, 0)] if n <= 4099 else [])
            for shift, ys_shift in variants:
                s = [SCALES[(j + shift) % 3] for j in range(m)]
                ys = None if ys_shift is None else [SCALES[(j + ys_shift) % 3] for j in range(m)]
                want = [((ys[j] if ys else 1.0) * y_host[j] - b_host[tb][j].astype(F64)) * s[j] for j in range(m)]
                sums = np.array([np.sum(w * w) for w in want])
                where = (n, str(np.dtype(tb)), m, shift)

                def reset():
                    for j in range(m):
                        ctx.copy(yy[j], y0[j])
                    ctx.synchronize()

                # the unfused sequence on this context
                reset()
                for j in range(m):
                    if ys and ys[j] != 1.0:
                        ctx.scal(ys[j], yy[j])
                    ctx.mx_axpy(-1.0, bb[j], yy[j])
                    ctx.scal(s[j], yy[j])
                # (every vector of the fused pass is compared with numpy below: long vectors save the downloads)
                ends = list(range(m)) if n <= 4099 else sorted({0, m - 1})
                seq = {j: yy[j].numpy() for j in ends}
                seq_dots = np.array([ctx.dot(v, v) for v in yy[:m]])
                # the fused pass
                reset()
                out, led = ledger_of(ctx, lambda: ctx.mx_rhs_residual_norms(bb[:m], s, yy[:m], ys))
                got = [v.numpy() for v in yy[:m]]
                for j in range(m):
                    assert np.array_equal(bits(got[j]), bits(want[j])), (where, j, "numpy")
                for j in ends:
                    assert np.array_equal(bits(got[j]), bits(seq[j])), (where, j, "sequence")
                    assert np.array_equal(bits(seq[j]), bits(want[j])), (where, j, "sequence against numpy")
                assert np.all(np.abs(out - sums) <= 64 * EPS * sums), (where, out, sums)
                if exact or m > K_OUTER_DST:  # the sequence's own dots
                    assert np.array_equal(bits(out), bits(seq_dots)), (where, out, seq_dots)
                if m <= K_OUTER_DST:
                    row = led.get("rhs_residual_norms")
                    assert row and row["calls"] == 1 and row["bytes"] == float(n * m * (16 + np.dtype(tb).itemsize)), (where, led)
                    assert set(led) == {"rhs_residual_norms"}, (where, sorted(led))
                # a repeat call gives the same bits
                reset()
                again = ctx.mx_rhs_residual_norms(bb[:m], s, yy[:m], ys)
                assert np.array_equal(bits(again), bits(out)), (where, again, out)
                for j in sorted({0, m - 1}):
                    assert np.array_equal(bits(yy[j].numpy()), bits(got[j])), (where, j, "repeat")
        for v in bb:
            v.free()
    for v in y0 + yy:
        v.free()


@pytest.mark.parametrize("n", [5, 4099])
@pytest.mark.parametrize("tb", [F32, F64], ids=["f32", "f64"])
def test_kernel_stores_a_pending_zero_fill_first(ctx, n, tb):
    y, z = ctx.upload(np.full(n, 3.0)), ctx.upload(np.full(n, 5.0))
    b = [ctx.upload(np.full(n, 1.0), tb), ctx.upload(np.full(n, 2.0), tb)]
    ctx.fill(0.0, y)  # recorded, not launched (csrc/pending_fill.h)
    out = ctx.mx_rhs_residual_norms(b, [2.0, 1.0], [y, z])
    assert np.array_equal(bits(y.numpy()), bits(np.full(n, -2.0))) and np.array_equal(z.numpy(), np.full(n, 3.0))
    assert np.array_equal(out, np.array([4.0 * n, 9.0 * n]))
    for v in [y, z] + b:
        v.free()


def test_kernel_arguments(ctx):
    import ctypes as C

    import subspace_hip as sh

    f = ctx.lib.ssp_mx_rhs_residual_norms
    y, z, b = ctx.upload(np.arange(8.0)), ctx.upload(np.ones(8)), ctx.upload(np.ones(8), F32)
    assert ctx.mx_rhs_residual_norms([], [], []).size == 0  # m = 0
    one = lambda v: (C.c_void_p * 1)(v.ptr if hasattr(v, "ptr") else v)  # noqa: E731
    s = (C.c_double * 2)(1.0, 1.0)
    out = (C.c_double * 2)(7.0, 7.0)
    assert f(ctx.handle, one(b), sh.SSP_F32, s, one(y), None, 1, 0, out) == 0 and out[0] == 0.0  # n = 0: zeros
    assert np.array_equal(y.numpy(), np.arange(8.0))
    assert f(ctx.handle, one(b), sh.SSP_F32, s, one(y), None, -1, 8, out) == 3
    assert b"negative" in ctx.lib.ssp_last_error()
    assert f(ctx.handle, one(b), 2, s, one(y), None, 1, 8, out) == 3  # not a dtype
    assert f(ctx.handle, one(b), sh.SSP_F32, None, one(y), None, 1, 8, out) == 3
    assert f(ctx.handle, one(b), sh.SSP_F32, s, one(y), None, 1, 8, None) == 3
    assert f(ctx.handle, one(0), sh.SSP_F32, s, one(y), None, 1, 8, out) == 3
    assert b"null vector" in ctx.lib.ssp_last_error()
    assert f(ctx.handle, one(b), sh.SSP_F32, s, one(0), None, 1, 8, out) == 3
    assert f(ctx.handle, one(b.ptr + 4), sh.SSP_F32, s, one(y), None, 1, 4, out) == 3
    assert b"16-byte aligned" in ctx.lib.ssp_last_error()
    assert f(ctx.handle, one(b), sh.SSP_F32, s, one(y.ptr + 8), None, 1, 4, out) == 3
    assert b"16-byte aligned" in ctx.lib.ssp_last_error()
    assert f(ctx.handle, one(y), sh.SSP_F64, s, one(y), None, 1, 8, out) == 3  # the destination is its right-hand side
    assert b"aliases" in ctx.lib.ssp_last_error()
    two_b, two_y = (C.c_void_p * 2)(z.ptr, y.ptr), (C.c_void_p * 2)(y.ptr, y.ptr)
    assert f(ctx.handle, two_b, sh.SSP_F64, s, two_y, None, 2, 8, out) == 3  # one destination twice
    two_y = (C.c_void_p * 2)(y.ptr, z.ptr)
    assert f(ctx.handle, two_b, sh.SSP_F64, s, two_y, None, 2, 8, out) == 3  # a destination is another's right-hand side
    assert np.array_equal(y.numpy(), np.arange(8.0)) and np.array_equal(z.numpy(), np.ones(8))
    with pytest.raises(TypeError):
        ctx.mx_rhs_residual_norms([y], [1.0], [b])  # the residuals are float64 vectors
    assert "ssp_mx_rhs_residual_norms" in sh.EXPORTS
    for v in (y, z, b):
        v.free()


# ---- 2, 3. the dense solves -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_3000():
    """tests/test_mixed_gpu.py dense_3000 with 3 right-hand sides from default_rng(11); |A|_2 and lambda_min."""
    n = 3000
    b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
    ev = np.linalg.eigvalsh(h)
    return h, np.random.default_rng(11).uniform(-1, 1, (3, n)), float(np.max(np.abs(ev))), float(ev[0])


def recompute_of(n, norm2, x, rhs):
    xn, bn = np.linalg.norm(x, axis=1), np.linalg.norm(rhs, axis=1)
    return n * EPS * (norm2 * xn + bn) / bn


def report(name, f64, ref, recompute):
    st = ref.get("refine") or {}
    print(f"\n{name}: iterations f64 {f64['iterations']} q32 {ref['iterations']}, refine {st}\n  errors {ref['errors']}\n"
          f"  residual norms {ref['residual_norms']}\n  f64 residual norms {f64['residual_norms']}\n  recompute {recompute}\n"
          f"  |x - x_f64| {np.linalg.norm(ref['x'] - f64['x'], axis=1)}")


def refined_criteria(name, f64, ref, threshold, rhs, norm2, lam_min):
    n, nrhs = rhs.shape[1], rhs.shape[0]
    recompute = recompute_of(n, norm2, ref["x"], rhs)
    report(name, f64, ref, recompute)
    assert f64["converged"] and ref["converged"]
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= threshold + recompute)
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= recompute)  # the errors are true residuals
    bound = (ref["residual_norms"] + f64["residual_norms"]) * np.linalg.norm(rhs, axis=1) / lam_min
    assert np.all(np.linalg.norm(ref["x"] - f64["x"], axis=1) <= bound)
    assert ref["iterations"] <= f64["iterations"] + 3
    assert 1 <= ref["refine"]["refined_actions"] <= nrhs * ref["iterations"]


@pytest.fixture(scope="module")
def dense_runs(ctx, dense_3000):
    import itsolv_hbm as ih

    h, rhs, _, _ = dense_3000
    kw = dict(convergence_threshold=1e-10, max_iter=60)
    return {"f64": ih.linear_equations_dense(ctx, h, rhs, **kw),
            "refined": ih.linear_equations_dense(ctx, h, rhs, q32=True, refine=True, **kw),
            "plain": ih.linear_equations_dense(ctx, h, rhs, q32=True, **kw),
            "f64_p8": ih.linear_equations_dense(ctx, h, rhs, max_p=8, **kw),
            "refined_p8": ih.linear_equations_dense(ctx, h, rhs, q32=True, refine=True, max_p=8, **kw)}


def test_dense_3000_refined_reaches_1e_10(dense_3000, dense_runs):
    _, rhs, norm2, lam_min = dense_3000
    refined_criteria("lineq dense_3000 at 1e-10", dense_runs["f64"], dense_runs["refined"], 1e-10, rhs, norm2, lam_min)


def test_dense_3000_refined_with_a_p_space(dense_3000, dense_runs):
    _, rhs, norm2, lam_min = dense_3000
    refined_criteria("lineq dense_3000 at 1e-10, max_p = 8", dense_runs["f64_p8"], dense_runs["refined_p8"], 1e-10, rhs,
                     norm2, lam_min)


def test_dense_3000_plain_q32_does_not_converge_at_1e_10(dense_runs):
    """Passes without the refined mode too: the stall the other cases are measured against."""
    plain = dense_runs["plain"]
    print(f"\nplain q32 lineq at 1e-10: iterations {plain['iterations']}, errors {plain['errors']}, residual norms "
          f"{plain['residual_norms']}")
    assert not plain["converged"]


def test_dense_3000_plain_q32_at_1e_6(ctx, dense_3000):
    import itsolv_hbm as ih

    h, rhs, norm2, _ = dense_3000
    n = h.shape[0]
    kw = dict(convergence_threshold=1e-6, max_iter=60)
    f64 = ih.linear_equations_dense(ctx, h, rhs, **kw)
    q32 = ih.linear_equations_dense(ctx, h, rhs, q32=True, **kw)
    k = q32["q_creations"] // 2  # the final Q size: every stored pair is a parameter and an action, nothing deleted
    xn, bn = np.linalg.norm(q32["x"], axis=1), np.linalg.norm(rhs, axis=1)
    bound = U32 * (norm2 * np.sqrt(k) * xn + bn) / bn + recompute_of(n, norm2, q32["x"], rhs)
    print(f"\nplain q32 lineq at 1e-6: iterations f64 {f64['iterations']} q32 {q32['iterations']}, Q size {k}\n  errors "
          f"{q32['errors']}\n  residual norms {q32['residual_norms']}\n  bound {bound}")
    assert f64["converged"] and q32["converged"]
    assert q32["iterations"] <= f64["iterations"] + 3
    assert np.all(np.abs(q32["errors"] - q32["residual_norms"]) <= bound)


# ---- 4. the bandwidth path, fused and call by call -----------------------------------------------------------------
SYNTH = dict(n=100_003, rho=0.1, rank=4, seed=20251015, nrhs=3, rhs_seed=11)
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import itsolv_hbm as ih
import subspace_hip as sh
S = json.loads(sys.argv[2])
out = {}
with sh.Context(0) as ctx:
    for name, extra in (("f64", {}), ("refined", dict(q32=True, refine=True))):
        ctx.ledger_reset()
        ctx.ledger_enable(True)
        r = ih.linear_equations_synth(ctx, S["n"], S["rho"], S["rank"], S["seed"], S["nrhs"], S["rhs_seed"],
                                      convergence_threshold=1e-8, **extra)
        ctx.synchronize()
        ctx.ledger_enable(False)
        out[name] = {"converged": bool(r["converged"]), "iterations": int(r["iterations"]),
                     "errors": [float(e) for e in r["errors"]], "residual_norms": [float(e) for e in r["residual_norms"]],
                     "refine": r.get("refine"), "x": [[float(v) for v in row] for row in r["x"]],
                     "calls": {op: v["calls"] for op, v in ctx.ledger().items()}}
print(json.dumps(out))
"""


def synth_solve(min_size):
    env = dict(os.environ, SSP_FUSED_MIN_SIZE=str(min_size))
    env.pop("SSP_ORTHO", None)
    env.pop("SSP_LEDGER_DETAIL", None)
    p = subprocess.run([sys.executable, "-c", CHILD, PKG, json.dumps(SYNTH)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    for r in out.values():
        for k in ("errors", "residual_norms", "x"):
            r[k] = np.array(r[k])
    return out


@pytest.fixture(scope="module")
def synth_solves():
    """(fused, call by call): each child runs the f64 and the refined solve; and the right-hand sides."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle

    rhs = np.array([oracle.random_vector(SYNTH["n"], SYNTH["rhs_seed"], r) for r in range(SYNTH["nrhs"])])
    return synth_solve(0), synth_solve(10**15), rhs


def named(calls, name):
    return sum(c for op, c in calls.items() if op.split("(")[0].split(" [")[0] == name)


def synth_criteria(name, run, rhs):
    # |H|_2 <= max d + rho |sum_l u_l u_l^T|_2 <= n + rho rank n; lambda_min >= min d = 1 (rho >= 0)
    norm2 = SYNTH["n"] * (1 + SYNTH["rho"] * SYNTH["rank"])
    refined_criteria(name, run["f64"], run["refined"], 1e-8, rhs, norm2, 1.0)


def test_synthetic_refined_on_the_fused_passes(synth_solves):
    fused, _, rhs = synth_solves
    synth_criteria("lineq synthetic 100003 at 1e-8, fused", fused, rhs)
    assert named(fused["refined"]["calls"], "rhs_residual_norms") > 0, fused["refined"]["calls"]
    assert named(fused["f64"]["calls"], "rhs_residual_norms") == 0, fused["f64"]["calls"]


def test_synthetic_refined_call_by_call(synth_solves):
    fused, plainly, rhs = synth_solves
    synth_criteria("lineq synthetic 100003 at 1e-8, call by call", plainly, rhs)
    for r in plainly.values():
        assert named(r["calls"], "rhs_residual_norms") == 0, r["calls"]
    assert plainly["refined"]["iterations"] == fused["refined"]["iterations"]


# ---- 5. the short-vector path --------------------------------------------------------------------------------------
def bh_problem():
    from test_solver_gpu import hamiltonian

    # the linear-equations fixture of tests/test_device_api_gpu.py (bh shifted, two right-hand sides), with the
    # shift that makes it positive definite (bh's lowest eigenvalue is near -25): lambda_min = 3
    h = hamiltonian("bh", 1e-8)
    h = h + (3.0 - float(np.linalg.eigvalsh((h + h.T) / 2)[0])) * np.eye(28)
    return h, np.vstack([h[:, 0] + 1.0, np.arange(1.0, 29.0)])


def test_short_vector_path_refined(ctx):
    import itsolv_hbm as ih

    h, rhs = bh_problem()
    ev = np.linalg.eigvalsh((h + h.T) / 2)
    assert ev[0] > 0
    kw = dict(convergence_threshold=1e-10)
    f64 = ih.linear_equations_dense(ctx, h, rhs, **kw)
    assert f64["converged"], "the f64 run must converge on bh at 1e-10 for this case to mean anything"
    ref = ih.linear_equations_dense(ctx, h, rhs, q32=True, refine=True, **kw)
    refined_criteria("lineq bh at 1e-10", f64, ref, 1e-10, rhs, float(np.max(np.abs(ev))), float(ev[0]))


# ---- 6. the reverse-communication API -----------------------------------------------------------------------------
@pytest.fixture()
def api(ctx):
    import iterative_solver

    iterative_solver.use_context(ctx)
    yield ctx
    iterative_solver.use_context(None)


def rc_run(api, h, rhs, options, device, refine):
    """One reverse-communication solve of A x = rhs at 1e-10 -> (result in refined_criteria's layout, the action)."""
    import device_api_cases as dc
    import iterative_solver
    import rc_refine_cases as rc

    nrhs, n = rhs.shape
    d = np.diag(h).copy()
    guess = sorted(np.argsort(d, kind="stable")[:nrhs])
    s = iterative_solver.LinearEquations(rhs, thresh=1e-10, hermitian=True, options=options)
    try:
        if s.q_storage == 4:
            d = rc.stored(d)
        target = dc.ViaDevice(s, api) if device else s
        _, _, nwork, act = rc.loop_refined(target, nrhs, n, lambda x: x @ h, d, guess, max_iter=60, refine=refine)
        errors = s.errors.copy()
        x, g = np.zeros((nrhs, n)), np.zeros((nrhs, n))
        target.solution(list(range(nrhs)), x, g)
        norms = np.linalg.norm(x @ h - rhs, axis=1) / np.linalg.norm(rhs, axis=1)
        return {"converged": bool(nwork == 0 and np.all(errors <= 1e-10)), "errors": errors, "residual_norms": norms,
                "iterations": s.statistics()["iterations"], "x": x, "refine": s.refine_statistics()}, act
    finally:
        s.finalize()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rc_refined_dense_3000_reaches_1e_10(api, dense_3000, device):
    h, rhs, norm2, lam_min = dense_3000
    f64, _ = rc_run(api, h, rhs, "", device, False)
    ref, act = rc_run(api, h, rhs, "Q_STORAGE=f32,Q_REFINE=1", device, True)
    refined_criteria(f"RC lineq dense_3000 at 1e-10, device={device}", f64, ref, 1e-10, rhs, norm2, lam_min)
    st = ref["refine"]
    assert st["refined_actions"] == sum(act.sizes) and max(act.sizes) <= 3 and st["max_delta"] > 0, (st, act.sizes)


# ---- 7. the refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,kw", [("hermitian", dict(hermitian=0)), ("max_size_qspace", dict(max_size_qspace=24)),
                                       ("reset_D", dict(reset_D=8)), ("augmented_hessian", dict(augmented_hessian=0.5))])
def test_refined_refuses_what_it_does_not_cover(ctx, option, kw):
    import itsolv_hbm as ih

    h, rhs = bh_problem()
    with pytest.raises(RuntimeError, match=option):
        ih.linear_equations_dense(ctx, h, rhs, q32=True, refine=True, **kw)
    assert ih.linear_equations_dense(ctx, h, rhs, q32=True, refine=True)["converged"]  # without the option it runs


def test_refine_needs_q32(ctx):
    import itsolv_hbm as ih

    h, rhs = bh_problem()
    with pytest.raises(ValueError, match="refine.*q32"):
        ih.linear_equations_dense(ctx, h, rhs, refine=True)
    with pytest.raises(ValueError, match="refine.*q32"):
        ih.linear_equations_synth(ctx, 64, 0.1, 1, 1, 2, 5, refine=True)


def test_rc_refusals_name_their_option(api):
    import iterative_solver

    h, rhs = bh_problem()
    for options, words, kw in (("Q_STORAGE=f32,Q_REFINE=1,Q_REFINE_DSPACE=1", ("Q_REFINE_DSPACE", "LinearEquations"), {}),
                               ("Q_REFINE=1", ("Q_REFINE", "LinearEquations"), {}),
                               ("Q_STORAGE=f32,Q_REFINE=1", ("refine", "hermitian"), dict(hermitian=False)),
                               ("Q_STORAGE=f32,Q_REFINE=1,MAX_SIZE_QSPACE=12", ("refine", "max_size_qspace"), {}),
                               ("Q_STORAGE=f32,Q_REFINE=1", ("refine", "augmented_hessian"), dict(aughes=0.5)),
                               ("Q_STORAGE=f32", ("Q_STORAGE=f32", "Davidson"), dict(algorithm="DIIS"))):
        args = dict(dict(hermitian=True), **kw)
        with pytest.raises(RuntimeError) as e:
            iterative_solver.LinearEquations(rhs, options=options, **args).finalize()
        assert all(w.lower() in str(e.value).lower() for w in words), (options, str(e.value))
    s = iterative_solver.LinearEquations(rhs, hermitian=True, options="Q_STORAGE=f32")  # the plain mode is admitted
    assert s.q_storage == 4
    s.finalize()
