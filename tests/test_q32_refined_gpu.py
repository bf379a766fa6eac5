"""The refined mode of the f32 Q space (include/itsolv_hbm.h *_q32_refined; itsolv_hbm/solvers.h set_refine):
Davidson with the Q space stored in 4 bytes per element reaching f64 thresholds.

1. ssp_quantise_f32 bit for bit against numpy's (x * s).astype(float32).astype(float64), and the three
   properties the scheme rests on (equal to the convert there and back, idempotent, a later convert exact);
2. the dense n = 3000 solve at 1e-10: converged, the solver's errors ARE the recomputed residual norms, the
   eigenvalues within the residual norms of the f64 run's, the iteration count within the q32 margin; the
   plain q32 solve of the same call does not converge (it passes without the feature: it shows that the
   other cases are not vacuous);
3. the synthetic solve at 1e-8 on the fused passes and call by call (child processes, SSP_FUSED_MIN_SIZE);
4. the short-vector path (fixture bh);
5. the refusals, each naming its option.
"""
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
F32, F64 = np.float32, np.float64
EXACT_MAX_DEFAULT = 2048  # ssp_ctx_set_exact_max default (include/subspace_hip.h)
FLT_MAX = float(np.finfo(F32).max)
FLT_TINY = float(np.finfo(F32).tiny)  # the smallest normal binary32

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, (1 << 20) + 5]
COUNTS = [1, 2, 3, 16, 17]
SCALES = [1.0, 0.3, -(2.0**-30)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def specials():
    """Products (x * s) the rounding has to get right: signed zeros, exact ties between two floats of both
    parities (the even neighbour below and above), values that land in binary32's subnormal range (ties
    there too, and below half the smallest subnormal), and magnitudes around FLT_MAX (the last is past the
    rounding boundary FLT_MAX + ulp / 2 and becomes inf)."""
    ulp1 = 2.0**-23
    sub = 2.0**-149  # the smallest subnormal
    p = [0.0, -0.0,
         1 + 0.5 * ulp1, 1 + 1.5 * ulp1, -(1 + 0.5 * ulp1), -(1 + 1.5 * ulp1),  # ties: to even below, above
         1 + 0.5 * ulp1 + 2.0**-52, 1 + 1.5 * ulp1 - 2.0**-52,  # one f64 ulp off a tie
         FLT_TINY / 2, FLT_TINY * (1 - 2.0**-30), 3.5 * sub, 2.5 * sub, 0.5 * sub, 0.5 * sub * (1 + 2.0**-50),
         -1.5 * sub, 0.25 * sub,
         FLT_MAX, FLT_MAX * (1 - 2.0**-30), FLT_MAX * (1 + 2.0**-30), -FLT_MAX * (1 + 2.0**-26),
         FLT_MAX * (1 + 2.0**-24), 1e39, -1e39]
    return np.array(p)


def inputs(n, m, s, seed):
    """m vectors of length n: uniform values with the specials planted as x = product / s (exact where s is a
    power of two; for another s the products land within an f64 ulp of the specials, and the specials
    themselves are planted too)."""
    r = np.random.default_rng(seed)
    sp = specials()
    exact = abs(s) == 2.0 ** round(np.log2(abs(s)))
    plant = sp / s if exact else np.concatenate([sp / s, sp])
    out = []
    for v in range(m):
        x = r.uniform(-2, 2, n) * 10.0 ** r.integers(-3, 4, n)
        k = min(n, plant.size)
        pos = r.permutation(n)[:k]
        x[pos] = np.roll(plant, v)[:k]
        out.append(x)
    return out


@pytest.fixture
def exact_max(ctx, request):
    ctx.set_exact_max(request.param)
    yield request.param
    ctx.set_exact_max(EXACT_MAX_DEFAULT)


# ---- 1. the quantise kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("exact_max", [EXACT_MAX_DEFAULT, 0], indirect=True, ids=["exact_default", "exact_0"])
def test_quantise_is_the_convert_there_and_back_bit_for_bit(ctx, exact_max, n):
    with np.errstate(over="ignore"):
        for s in SCALES:
            xs = inputs(n, max(COUNTS), s, seed=n)
            want = [(x * s).astype(F32).astype(F64) for x in xs]
            if n >= 23:  # every special fits: the planted classes are really there
                w0 = want[0]
                assert np.any(np.isinf(w0)) and np.any(np.signbit(w0) & (w0 == 0))
                assert np.any((np.abs(w0) > 0) & (np.abs(w0) < FLT_TINY)) and np.any(np.abs(w0) == FLT_MAX)
            t32, back = ctx.alloc(n, F32), ctx.alloc(n)
            for m in COUNTS:
                dev = [ctx.upload(x) for x in xs[:m]]
                ctx.ledger_reset()
                ctx.ledger_enable(True)
                ctx.quantise_f32(dev, [s] * m)
                ctx.synchronize()
                led = ctx.ledger()
                ctx.ledger_enable(False)
                assert led["quantise_f32"]["calls"] == 1 and led["quantise_f32"]["bytes"] == 16.0 * m * n, led
                got = [v.numpy() for v in dev]
                for v in range(m):
                    assert np.array_equal(bits(got[v]), bits(want[v])), (n, m, s, v)
                for v in sorted({0, m - 1}):
                    # equal to the narrowing convert (scale s) and back, on the same input
                    src = ctx.upload(xs[v])
                    ctx.mx_copy(t32, src, s)
                    ctx.mx_copy(back, t32)
                    assert np.array_equal(bits(back.numpy()), bits(got[v])), (n, m, s, v)
                    src.free()
                    # a following convert to f32 and back returns the vector unchanged
                    ctx.mx_copy(t32, dev[v])
                    ctx.mx_copy(back, t32)
                    assert np.array_equal(bits(back.numpy()), bits(got[v])), (n, m, s, v)
                # idempotent
                ctx.quantise_f32(dev)
                for v in range(m):
                    assert np.array_equal(bits(dev[v].numpy()), bits(got[v])), (n, m, s, v)
                for v in dev:
                    v.free()
            t32.free()
            back.free()


@pytest.mark.parametrize("n", [5, 4099])
def test_quantise_stores_a_pending_zero_fill_first(ctx, n):
    v, w = ctx.upload(np.full(n, 1 + 2.0**-30)), ctx.upload(np.full(n, 3 + 2.0**-30))
    ctx.fill(0.0, v)  # recorded, not launched (csrc/pending_fill.h)
    ctx.quantise_f32([v, w], [0.5, 1.0])
    assert np.array_equal(bits(v.numpy()), bits(np.zeros(n)))
    assert np.array_equal(w.numpy(), np.full(n, 3.0))
    v.free()
    w.free()


def test_quantise_arguments(ctx):
    import ctypes as C

    import subspace_hip as sh

    x = ctx.upload(np.arange(8.0))
    ctx.quantise_f32([])  # m = 0
    one = (C.c_void_p * 1)(x.ptr)
    assert ctx.lib.ssp_quantise_f32(ctx.handle, one, None, 1, 0) == 0  # n = 0
    assert np.array_equal(x.numpy(), np.arange(8.0))
    assert ctx.lib.ssp_quantise_f32(ctx.handle, one, None, -1, 8) == 3
    off = (C.c_void_p * 1)(x.ptr + 8)
    assert ctx.lib.ssp_quantise_f32(ctx.handle, off, None, 1, 4) == 3  # not 16-byte aligned
    assert b"16-byte aligned" in ctx.lib.ssp_last_error()
    with pytest.raises(TypeError):
        q = ctx.upload(np.ones(8), F32)
        try:
            ctx.quantise_f32([q])
        finally:
            q.free()
    assert "ssp_quantise_f32" in sh.EXPORTS
    x.free()


# ---- 2. the solves ------------------------------------------------------------------------------------------
def report(name, f64, ref):
    st = ref["refine"]
    print(f"\n{name}: iterations f64 {f64['iterations']} refined {ref['iterations']} (difference "
          f"{ref['iterations'] - f64['iterations']}), refined actions {st['refined_actions']}, first refined iteration "
          f"{st['first_refined_iteration']}, max delta {st['max_delta']:.3e}\n  errors {ref['errors']}\n  residual norms "
          f"{ref['residual_norms']}\n  f64 residual norms {f64['residual_norms']}\n  eigenvalue differences "
          f"{np.abs(ref['eigenvalues'] - f64['eigenvalues'])}")


def refined_criteria(name, f64, ref, threshold, recompute, nroots):
    """recompute: the worst-case rounding of the runner's recomputation of a residual norm, n eps64 |H|_2."""
    report(name, f64, ref)
    assert f64["converged"] and ref["converged"]
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= threshold + recompute)
    # the solver's own errors are true residuals now
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= recompute)
    # hermitian H: each Ritz value lies within its residual norm of an eigenvalue
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])
    assert ref["iterations"] <= f64["iterations"] + 3
    st = ref["refine"]
    assert 1 <= st["refined_actions"] <= nroots * ref["iterations"]
    assert st["first_refined_iteration"] >= 2


@pytest.fixture(scope="module")
def dense_3000():
    """tests/test_mixed_gpu.py dense_3000: H = (B + B^T) / 2 with B uniform(-0.01, 0.01), diagonal
    1 + 9 i / n; and |H|_2."""
    n = 3000
    b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
    return h, float(np.max(np.abs(np.linalg.eigvalsh(h))))


@pytest.fixture(scope="module")
def dense_runs(ctx, dense_3000):
    import itsolv_hbm as ih

    h, _ = dense_3000
    kw = dict(nroots=3, convergence_threshold=1e-10, max_iter=60)
    return (ih.davidson_dense(ctx, h, **kw), ih.davidson_dense(ctx, h, q32=True, refine=True, **kw),
            ih.davidson_dense(ctx, h, q32=True, **kw))


def test_dense_3000_refined_reaches_1e_10(dense_3000, dense_runs):
    h, norm2 = dense_3000
    f64, ref, _ = dense_runs
    refined_criteria("dense_3000 at 1e-10", f64, ref, 1e-10, h.shape[0] * EPS * norm2, 3)


def test_dense_3000_plain_q32_does_not_converge_at_1e_10(dense_runs):
    """Passes without the refined mode too: the stall the other cases are measured against."""
    plain = dense_runs[2]
    print(f"\nplain q32 at 1e-10: iterations {plain['iterations']}, errors {plain['errors']}, residual norms "
          f"{plain['residual_norms']}")
    assert not plain["converged"]


def test_short_vector_path_refined(ctx):
    """Fixture bh (n = 28: every vector on the short-vector path) with 2 roots at 1e-10."""
    import itsolv_hbm as ih
    from test_solver_gpu import hamiltonian

    h = hamiltonian("bh", 1e-8)
    kw = dict(nroots=2, convergence_threshold=1e-10)
    f64 = ih.davidson_dense(ctx, h, **kw)
    assert f64["converged"], "the f64 run must converge on bh at 1e-10 for this case to mean anything"
    ref = ih.davidson_dense(ctx, h, q32=True, refine=True, **kw)
    norm2 = float(np.max(np.abs(np.linalg.eigvalsh((h + h.T) / 2))))
    refined_criteria("bh at 1e-10", f64, ref, 1e-10, h.shape[0] * EPS * norm2, 2)


# ---- 3. the bandwidth path, fused and call by call ----------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import itsolv_hbm as ih
import subspace_hip as sh
max_p = int(sys.argv[2])
REDUCING = ("dot", "gemm_inner", "axpy_inner", "scal_inner", "axpy_norm", "axpy_gram", "axpy_pairs_norm", "select",
            "gemm_inner_sparse", "gemm_inner_f32", "dot_f32", "gemm_inner_cols")
kw = dict(nroots=4, convergence_threshold=1e-8)
if max_p:
    kw["max_p"] = max_p
out = {}
with sh.Context(0) as ctx:
    for name, extra in (("f64", {}), ("refined", dict(q32=True, refine=True)),
                        ("plain", dict(q32=True, convergence_threshold=1e-6))):
        ctx.ledger_reset()
        ctx.ledger_enable(True)
        r = ih.davidson_synthetic(ctx, 100_003, 0.1, 2, 20251015, **dict(kw, **extra))
        ctx.synchronize()
        ctx.ledger_enable(False)
        calls = {op: v["calls"] for op, v in ctx.ledger().items()}
        out[name] = {"converged": bool(r["converged"]), "iterations": int(r["iterations"]),
                     "eigenvalues": [float(e) for e in r["eigenvalues"]], "errors": [float(e) for e in r["errors"]],
                     "residual_norms": [float(e) for e in r["residual_norms"]], "refine": r.get("refine"),
                     "reducing": sum(c for op, c in calls.items() if op.split("(")[0].split(" [")[0] in REDUCING),
                     "calls": calls}
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
    """(fused, call by call) of one problem: each child runs the f64, the refined and (at 1e-6) the plain solve."""
    return solve(request.param, 0), solve(request.param, 10**15)


def synth_criteria(name, run):
    f64, ref = run["f64"], run["refined"]
    report(name, f64, ref)
    assert f64["converged"] and ref["converged"]
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])
    assert ref["iterations"] <= f64["iterations"] + 3
    st = ref["refine"]
    assert 1 <= st["refined_actions"] <= 4 * ref["iterations"]
    assert st["first_refined_iteration"] >= 2


def test_synthetic_refined_on_the_fused_passes(solves):
    synth_criteria("synthetic 100003 at 1e-8, fused", solves[0])
    ref, plain = solves[0]["refined"], solves[0]["plain"]
    calls = ref["calls"]
    # the new rows of every add_vector are one mixed inner product (no Q actions among its columns), and the
    # overlaps of propose_rspace one more: what the plain q32 solve issues per iteration
    # (an iteration with an empty Q space or an empty working set has all-f64 columns or no rows: the same few
    # in both solves)
    assert 0 < calls.get("gemm_inner_cols", 0) <= 2 * ref["iterations"], calls
    assert calls["gemm_inner_cols"] - 2 * ref["iterations"] == plain["calls"]["gemm_inner_cols"] - 2 * plain["iterations"]
    assert 0 < calls.get("quantise_f32", 0) <= ref["iterations"], calls
    # no more reducing calls per iteration than the plain q32 solve, apart from the refined residuals' (one
    # fused residual-and-norms pass per iteration that refined)
    per_ref = (ref["reducing"] - (ref["iterations"] - ref["refine"]["first_refined_iteration"] + 1)) / ref["iterations"]
    per_plain = plain["reducing"] / plain["iterations"]
    print(f"\nreducing calls per iteration: refined {per_ref:.2f} (+ the refined residuals), plain q32 {per_plain:.2f}"
          f"\nrefined calls {calls}\nplain calls {plain['calls']}")
    assert per_ref <= per_plain


def test_synthetic_refined_call_by_call(solves):
    synth_criteria("synthetic 100003 at 1e-8, call by call", solves[1])
    assert solves[1]["refined"]["calls"].get("gemm_inner_cols", 0) == 0
    assert solves[1]["refined"]["iterations"] == solves[0]["refined"]["iterations"]


# ---- 5. refusals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,kw", [("max_size_qspace", dict(max_size_qspace=24)), ("reset_D", dict(reset_D=8)),
                                       ("hermitian", dict(hermitian=0))])
def test_refined_refuses_what_it_does_not_cover(ctx, option, kw):
    import itsolv_hbm as ih

    h = np.diag(np.arange(1.0, 41.0)) + 0.01
    with pytest.raises(RuntimeError, match=option):
        ih.davidson_dense(ctx, h, q32=True, refine=True, nroots=2, **kw)
    r = ih.davidson_dense(ctx, h, q32=True, refine=True, nroots=2)  # the same call without the option runs
    assert r["converged"]


def test_refine_needs_q32(ctx):
    import itsolv_hbm as ih

    with pytest.raises(ValueError, match="refine.*q32"):
        ih.davidson_dense(ctx, np.eye(4), refine=True, nroots=1)
    with pytest.raises(ValueError, match="refine.*q32"):
        ih.davidson_synthetic(ctx, 64, 0.1, 1, 1, refine=True)
