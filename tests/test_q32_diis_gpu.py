"""DIIS with its history stored as f32 differences behind f64 anchors (include/subspace_hip.h
ssp_q32_store_differences, ssp_q32_anchor_combine; itsolv_hbm/diis_differences.h; include/itsolv_hbm.h
itsolv_diis_*_q32; Q_STORAGE=f32 of IterativeSolverNonLinearEquationsInitialize).

1. the two passes, bit for bit their unfused sequences on the same context: ssp_copy to scratch, ssp_axpy(-1),
   ssp_mx_copy to f32 and ssp_copy to the anchor for the store; ssp_copy of the anchor and ssp_mx_gemm_outer
   (alphas = -gamma, F32 -> F64, set = 0) for the combination -- at the lengths of tests/test_q32_lineq_gpu.py,
   k in {0, 1, 3, 4, 5, 17, 65} (65: one more than a gemm_outer launch takes), m in {1, 2} panels and {1, 2, 16}
   vectors, exact_max at its default and at 0; the ledger rows; pending zero fills; the argument errors;
2. diis_synthetic on C5 at n = 100003 and 1e-8, q32 against f64 in one process, on the fused passes and call by
   call (child processes, SSP_FUSED_MIN_SIZE), without a limit and with max_size_qspace = 5; the history's bytes;
   the ledger; and the same at 1e-10 and 1e-12, where only the final residual is held against the f64 solve's;
3. diis_dense on dense_3000 at 1e-8 in the same children, with the same criteria;
4. a short-vector solve (n <= exact_max) whose fused and call-by-call paths agree bit for bit;
5. the reverse-communication loop of tests/test_reverse_comm.py's NonLinearEquations case with Q_STORAGE=f32, the
   host and the device route bit for bit;
6. the refusals, each naming its option and the family.

Criteria of a q32 solve against the f64 solve of the same problem: both converge, the q32 solve in at most one
iteration more (tests/test_q32_diis_model.py (b)), and the residual recomputed in f64 from its final parameters is
below the threshold."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in cast")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "iterative-solver_amd")
F32, F64 = np.float32, np.float64
EXACT_MAX_DEFAULT = 2048  # ssp_ctx_set_exact_max default (include/subspace_hip.h)
K_OUTER_SRC = 64  # sources per ssp_mx_gemm_outer launch

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, (1 << 20) + 5]
KS = [0, 1, 3, 4, 5, 17, K_OUTER_SRC + 1]


def test_the_lengths_are_those_of_the_linear_equations_kernel_tests():
    from test_q32_lineq_gpu import LENGTHS as theirs

    assert LENGTHS == theirs


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


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


def wide(rng, n):
    return rng.uniform(-2, 2, n) * 10.0 ** rng.integers(-3, 4, n)


# ---- 1. the two passes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("exact_max", [EXACT_MAX_DEFAULT, 0], indirect=True, ids=["exact_default", "exact_0"])
def test_store_differences_is_the_unfused_sequence_bit_for_bit(ctx, exact_max, n):
    rng = np.random.default_rng(n)
    mmax = 16
    a_host = [wide(rng, n) for _ in range(mmax)]
    # new points near the anchors (differences 1e-9 of the values: what a converging history stores), far from them,
    # and equal to them
    v_host = [a * (1 + 1e-9 * rng.uniform(-1, 1, n)) if j % 3 == 0 else wide(rng, n) if j % 3 == 1 else a.copy()
              for j, a in enumerate(a_host)]
    vv = [ctx.upload(v) for v in v_host]
    a0 = [ctx.upload(a) for a in a_host]  # pristine anchors: every run starts from a device copy of these
    aa, dd = [ctx.alloc(n) for _ in range(mmax)], [ctx.alloc(n, F32) for _ in range(mmax)]
    t, d_seq = ctx.alloc(n), ctx.alloc(n, F32)
    for m in (1, 2, 16):
        ends = list(range(m)) if n <= 4099 else sorted({0, m - 1})
        want_d = {j: (v_host[j] - a_host[j]).astype(F32) for j in ends}
        seq = {}
        for j in ends:  # the unfused sequence on this context
            ctx.copy(aa[j], a0[j])
            ctx.copy(t, vv[j])
            ctx.axpy(-1.0, aa[j], t)
            ctx.mx_copy(d_seq, t)
            ctx.copy(aa[j], vv[j])
            seq[j] = (d_seq.numpy(), aa[j].numpy())
        for j in range(m):
            ctx.copy(aa[j], a0[j])
            ctx.fill(-7.0, dd[j])
        ctx.synchronize()
        _, led = ledger_of(ctx, lambda: ctx.q32_store_differences(vv[:m], aa[:m], dd[:m]))
        for j in ends:
            where = (n, m, j)
            got_d, got_a = dd[j].numpy(), aa[j].numpy()
            assert np.array_equal(bits(got_d), bits(seq[j][0])), (where, "differences against the sequence")
            assert np.array_equal(bits(got_a), bits(seq[j][1])), (where, "anchors against the sequence")
            assert np.array_equal(bits(got_d), bits(want_d[j])), (where, "differences against numpy")
            assert np.array_equal(bits(got_a), bits(v_host[j])), (where, "anchors against numpy")
        row = led.get("store_differences_f32")
        assert row and row["calls"] == 1 and row["bytes"] == float(28 * n * m), (n, m, led)
        assert set(led) == {"store_differences_f32"}, (n, m, sorted(led))
    # a null dd refreshes the anchors only
    ctx.copy(aa[0], a0[0])
    ctx.q32_store_differences(vv[:1], aa[:1], None)
    assert np.array_equal(bits(aa[0].numpy()), bits(v_host[0]))
    for v in vv + a0 + aa + dd + [t, d_seq]:
        v.free()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("exact_max", [EXACT_MAX_DEFAULT, 0], indirect=True, ids=["exact_default", "exact_0"])
def test_anchor_combine_is_the_unfused_sequence_bit_for_bit(ctx, exact_max, n):
    rng = np.random.default_rng(1000 + n)
    kmax = max(KS)
    pool_host = [wide(rng, n).astype(F32) for _ in range(kmax + 1)]
    pool = [ctx.upload(d, F32) for d in pool_host]  # panel j reads pool[j : j + k]: the panels' sources differ
    a_host = [wide(rng, n), wide(rng, n)]
    aa = [ctx.upload(a) for a in a_host]
    yy, y_seq = [ctx.alloc(n), ctx.alloc(n)], ctx.alloc(n)
    exact = 0 < n <= exact_max
    for k in KS:
        gam = rng.uniform(-1.5, 1.5, k)
        if k:
            gam[0] = 0.0 if k > 3 else gam[0]  # (a converged step's coefficients are zeros)
        for m in (1, 2):
            where = (n, k, m)
            seq = []
            for j in range(m):  # the unfused sequence on this context
                ctx.copy(y_seq, aa[j])
                if k:
                    ctx.mx_gemm_outer(-gam.reshape(k, 1), pool[j:j + k], [y_seq])
                seq.append(y_seq.numpy())
            for j in range(m):
                ctx.fill(-7.0, yy[j])
            ctx.synchronize()
            _, led = ledger_of(ctx, lambda: ctx.q32_anchor_combine(gam, aa[:m], [pool[j:j + k] for j in range(m)], yy[:m]))
            for j in range(m):
                got = yy[j].numpy()
                assert np.array_equal(bits(got), bits(seq[j])), (where, j, "sequence")
                ref = a_host[j] - sum((g * pool_host[j + i].astype(F64) for i, g in enumerate(gam)), np.zeros(n))
                scale = np.abs(a_host[j]) + sum((abs(g) * np.abs(pool_host[j + i]) for i, g in enumerate(gam)), np.zeros(n))
                assert np.all(np.abs(got - ref) <= 4 * (k + 1) * np.finfo(F64).eps * scale), (where, j, "numpy")
            if k and not exact:
                row = led.get("anchor_combine_f32")
                assert row and row["calls"] == 1 and row["bytes"] == float(n * m * (16 + 4 * k)), (where, led)
                assert set(led) == {"anchor_combine_f32"}, (where, sorted(led))
            else:  # a copy (k = 0), or the sequence itself on the exact path
                assert "anchor_combine_f32" not in led, (where, sorted(led))
    for v in pool + aa + yy + [y_seq]:
        v.free()


@pytest.mark.parametrize("n", [5, 4099])
def test_pending_zero_fills_of_sources_are_stored_and_of_destinations_dropped(ctx, n):
    v, a = ctx.upload(np.full(n, 3.0)), ctx.upload(np.full(n, 5.0))
    d = ctx.alloc(n, F32)
    ctx.fill(0.0, v)  # recorded, not launched (csrc/pending_fill.h): a source
    ctx.q32_store_differences([v], [a], [d])
    assert np.array_equal(d.numpy(), np.full(n, -5.0, F32)) and np.array_equal(a.numpy(), np.zeros(n))
    ctx.upload_into(v, np.full(n, 3.0))
    ctx.upload_into(a, np.full(n, 5.0))
    ctx.fill(0.0, a)  # the anchor: read, then written
    ctx.q32_store_differences([v], [a], [d])
    assert np.array_equal(d.numpy(), np.full(n, 3.0, F32)) and np.array_equal(a.numpy(), np.full(n, 3.0))
    # the store's write-only destination over f64 blocks with a pending zero fill: one that lies inside the
    # difference's bytes (dropped) and one that reaches beyond them (stored first: its other bytes stay zeros)
    import subspace_hip as sh

    ctx.upload_into(a, np.full(n, 5.0))
    for block in ((n + 1) // 2 if n % 2 == 0 else n // 2, n):
        if block == 0:
            continue
        z = ctx.upload(np.full(block, 9.0))
        ctx.fill(0.0, z)
        over = sh.DeviceVector(ctx, min(n, 2 * block), z.ptr, owner=False, dtype=F32)  # the f32 vector placed over z
        m = over.n
        v2, a2 = ctx.upload(np.full(m, 3.0)), ctx.upload(np.full(m, 5.0))
        ctx.q32_store_differences([v2], [a2], [over])
        ctx.scal(1.0, v2)  # an entry point that stores every pending fill: none may land on the differences now
        assert np.array_equal(over.numpy(), np.full(m, -2.0, F32)), (n, block)
        tail = z.numpy()[(m + 1) // 2:]
        assert np.array_equal(tail, np.zeros(tail.size)), (n, block)
        for x in (z, v2, a2):
            x.free()
    y = ctx.upload(np.full(n, 9.0))
    ctx.upload_into(d, np.full(n, 2.0, F32))
    ctx.fill(0.0, a)  # a source of the combination
    ctx.fill(0.0, y)  # its destination: written in full, the fill must not land on the result
    ctx.q32_anchor_combine([0.5], [a], [[d]], [y])
    ctx.synchronize()
    assert np.array_equal(y.numpy(), np.full(n, -1.0))
    ctx.scal(1.0, y)  # an entry point that stores every pending fill
    assert np.array_equal(y.numpy(), np.full(n, -1.0))
    for x in (v, a, d, y):
        x.free()


def test_arguments(ctx):
    import subspace_hip as sh

    st, co = ctx.lib.ssp_q32_store_differences, ctx.lib.ssp_q32_anchor_combine
    err = lambda: ctx.lib.ssp_last_error()  # noqa: E731
    v, a, y = ctx.upload(np.arange(8.0)), ctx.upload(np.ones(8)), ctx.upload(np.full(8, 4.0))
    d, e = ctx.upload(np.full(8, 2.0), F32), ctx.upload(np.full(8, 3.0), F32)
    ptrs = lambda *vs: (C.c_void_p * len(vs))(*[x.ptr if hasattr(x, "ptr") else x for x in vs])  # noqa: E731
    g = (C.c_double * 2)(1.0, 1.0)
    untouched = lambda: (np.array_equal(v.numpy(), np.arange(8.0)) and np.array_equal(a.numpy(), np.ones(8))  # noqa: E731
                         and np.array_equal(y.numpy(), np.full(8, 4.0)) and np.array_equal(d.numpy(), np.full(8, 2.0, F32)))
    # m = 0 and n = 0 return at once
    assert st(ctx.handle, None, None, None, 0, 8) == 0 and st(ctx.handle, ptrs(v), ptrs(a), ptrs(d), 1, 0) == 0
    assert co(ctx.handle, g, None, None, 1, None, 0, 8) == 0 and co(ctx.handle, g, ptrs(a), ptrs(d), 1, ptrs(y), 1, 0) == 0
    ctx.q32_store_differences([], [], [])
    ctx.q32_anchor_combine([], [], [], [])
    assert untouched()
    # negative dimensions, null lists and vectors, alignment
    assert st(ctx.handle, ptrs(v), ptrs(a), ptrs(d), -1, 8) == 3 and b"negative" in err()
    assert co(ctx.handle, g, ptrs(a), ptrs(d), -1, ptrs(y), 1, 8) == 3 and b"negative" in err()
    assert co(ctx.handle, g, ptrs(a), ptrs(d), 1, ptrs(y), -1, 8) == 3 and b"negative" in err()
    assert st(ctx.handle, None, ptrs(a), ptrs(d), 1, 8) == 3 and b"null vector list" in err()
    assert st(ctx.handle, ptrs(0), ptrs(a), ptrs(d), 1, 8) == 3 and b"null vector" in err()
    assert co(ctx.handle, g, ptrs(a), ptrs(0), 1, ptrs(y), 1, 8) == 3 and b"null vector" in err()
    assert co(ctx.handle, None, ptrs(a), ptrs(d), 1, ptrs(y), 1, 8) == 3 and b"null gammas" in err()
    assert st(ctx.handle, ptrs(v.ptr + 8), ptrs(a), ptrs(d), 1, 4) == 3 and b"16-byte aligned" in err()
    assert st(ctx.handle, ptrs(v), ptrs(a), ptrs(d.ptr + 4), 1, 4) == 3 and b"16-byte aligned" in err()
    assert co(ctx.handle, g, ptrs(a), ptrs(d), 1, ptrs(y.ptr + 8), 1, 4) == 3 and b"16-byte aligned" in err()
    # aliasing is refused, not undefined
    assert st(ctx.handle, ptrs(v), ptrs(v), ptrs(d), 1, 8) == 3 and b"aliases" in err()  # the anchor is the point
    assert st(ctx.handle, ptrs(v), ptrs(a), ptrs(a), 1, 8) == 3 and b"aliases" in err()  # the difference is the anchor
    assert st(ctx.handle, ptrs(v), ptrs(a), ptrs(v), 1, 8) == 3 and b"aliases" in err()  # the difference is the point
    assert st(ctx.handle, ptrs(v, y), ptrs(a, a), ptrs(d, e), 2, 8) == 3 and b"same vector" in err()  # one anchor twice
    assert st(ctx.handle, ptrs(v, y), ptrs(a, v), ptrs(d, e), 2, 8) == 3 and b"aliases" in err()  # an anchor is another's point
    assert st(ctx.handle, ptrs(v, v), ptrs(a, y), ptrs(d, d), 2, 8) == 3 and b"same vector" in err()  # one difference twice
    assert co(ctx.handle, g, ptrs(a), ptrs(d), 1, ptrs(a), 1, 8) == 3 and b"aliases" in err()  # the destination is its anchor
    assert co(ctx.handle, g, ptrs(a), ptrs(d), 1, ptrs(d), 1, 8) == 3 and b"aliases" in err()  # ... a difference
    assert co(ctx.handle, g, ptrs(a, v), ptrs(d, e), 1, ptrs(y, y), 2, 8) == 3 and b"same vector" in err()  # one destination twice
    assert co(ctx.handle, g, ptrs(a, y), ptrs(d, e), 1, ptrs(y, v), 2, 8) == 3 and b"aliases" in err()  # ... another's anchor
    assert untouched()
    with pytest.raises(TypeError):
        ctx.q32_store_differences([v], [a], [y])  # the differences are float32 vectors
    with pytest.raises(TypeError):
        ctx.q32_anchor_combine([1.0], [a], [[y]], [v])
    with pytest.raises(ValueError):
        ctx.q32_anchor_combine([1.0, 2.0], [a], [[d]], [y])  # one coefficient per difference
    assert {"ssp_q32_store_differences", "ssp_q32_anchor_combine"} == set(sh.OPTIONAL_DIIS) <= set(sh.EXPORTS)
    for x in (v, a, y, d, e):
        x.free()


# ---- 2, 4. the synthetic solves, fused and call by call ------------------------------------------------------------
N_C5, N_SHORT, N_DENSE = 100_003, 2000, 3000
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import itsolv_hbm as ih
import subspace_hip as sh
out = {}
def dense_3000():  # tests/test_mixed_gpu.py dense_3000
    n = 3000
    b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
    return h
with sh.Context(0) as ctx:
    for name, n, kw in json.loads(sys.argv[2]):
        for q32 in (False, True):
            ctx.ledger_reset()
            ctx.ledger_enable(True)
            if name.startswith("dense"):
                r = ih.diis_dense(ctx, dense_3000(), q32=q32, max_iter=60, **kw)
            else:
                r = ih.diis_synthetic(ctx, n, **ih.c5_spec(n), q32=q32, max_iter=60, **kw)
            ctx.synchronize()
            ctx.ledger_enable(False)
            out[name + ("/q32" if q32 else "/f64")] = {
                "converged": bool(r["converged"]), "iterations": int(r["iterations"]), "r_creations": int(r["r_creations"]),
                "errors": [float(e) for e in r["errors"]], "residual_norms": [float(e) for e in r["residual_norms"]],
                "diis_q32": r.get("diis_q32"), "x": r["x"].tobytes().hex(), "nq": [int(v) for v in r["trace"]["nq"]],
                "calls": {op: v["calls"] for op, v in ctx.ledger().items()}}
print(json.dumps(out))
"""
CASES = [["1e-8", N_C5, dict(convergence_threshold=1e-8)],
         ["1e-8 max_size_qspace=5", N_C5, dict(convergence_threshold=1e-8, max_size_qspace=5)],
         ["1e-10", N_C5, dict(convergence_threshold=1e-10)],
         ["1e-12", N_C5, dict(convergence_threshold=1e-12)],
         ["short", N_SHORT, dict(convergence_threshold=1e-8)],
         ["dense 1e-8", N_DENSE, dict(convergence_threshold=1e-8)],
         ["dense 1e-8 max_size_qspace=5", N_DENSE, dict(convergence_threshold=1e-8, max_size_qspace=5)]]


def child_solves(min_size):
    env = dict(os.environ, SSP_FUSED_MIN_SIZE=str(min_size))
    env.pop("SSP_LEDGER_DETAIL", None)
    p = subprocess.run([sys.executable, "-c", CHILD, PKG, json.dumps(CASES)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    for r in out.values():
        r["x"] = np.frombuffer(bytes.fromhex(r["x"]), dtype=F64)
    return out


@pytest.fixture(scope="module")
def solves():
    """(fused, call by call): each child runs every case in f64 and in q32 on one context."""
    return child_solves(0), child_solves(10**15)


def c5_residual(x):
    """|H (x - t 1)| of itsolv_hbm/problems.h c5_spec (rank 1), in numpy from x."""
    n = x.size
    g = np.arange(n, dtype=F64) * 0.6180339887498949  # kPhi1, (sqrt(5) - 1) / 2
    d = 1.0 + 2.0 * (g - np.floor(g))
    e = x - 1.0 / np.sqrt(n)
    return float(np.linalg.norm(d * e + np.sum(e) / n))


def named(calls, name):
    return sum(c for op, c in calls.items() if op.split("(")[0].split(" [")[0] == name)


def dense_residual(x):
    """|H (x - 1)| of the dense problem (host/capi_problems.h DenseProblem), in numpy from x."""
    b = np.random.default_rng(7).uniform(-1, 1, (N_DENSE, N_DENSE)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(N_DENSE), np.arange(N_DENSE)] = 1 + 9 * np.arange(N_DENSE) / N_DENSE
    return float(np.linalg.norm(h @ (x - 1.0)))


def solve_criteria(name, f64, q32, threshold, residual=c5_residual):
    res = residual(q32["x"])
    print(f"\n{name}: iterations f64 {f64['iterations']} q32 {q32['iterations']}, q32 error {q32['errors'][0]:.3e}, residual "
          f"recomputed on the device {q32['residual_norms'][0]:.3e} and in numpy {res:.3e}; f64 residual "
          f"{f64['residual_norms'][0]:.3e}; history {q32['diis_q32']}")
    assert f64["converged"] and q32["converged"]
    assert q32["iterations"] <= f64["iterations"] + 1
    assert q32["residual_norms"][0] < threshold and res < threshold
    return res


def history_and_ledger(f64, q32, n, case, path):
    # the history: k - 1 pairs of f32 differences and two f64 anchors, (k - 1) 8 n + 16 n bytes up to the arena's
    # rounding of each of its 2 k blocks to 256 bytes
    st = q32["diis_q32"]
    k = st["points"]
    assert k == q32["nq"][-1] and st["pairs"] == k - 1 and k >= 2
    if "max_size_qspace" in case:
        assert max(q32["nq"]) <= 5
    assert abs(st["history_bytes"] - ((k - 1) * 8 * n + 16 * n)) <= 2 * k * 256, st
    # the passes: every point after the first is stored by one store_differences and gives H its row by one
    # gemm_inner_cols, and every construction from two or more points is one anchor_combine: one per add_vector
    # after the first (both vectors in it), one per end_iteration that has a working set to rebuild after the first
    # (the preconditioned ones: an extrapolated residual under the threshold leaves none, as in the f64 solver), and
    # the final solution; call by call there is neither
    points = q32["r_creations"]
    calls = q32["calls"]
    print(sorted(calls.items()))
    if path == 0:
        assert named(calls, "store_differences_f32") == points - 1, sorted(calls.items())
        assert named(calls, "gemm_inner_cols") == points - 1, sorted(calls.items())
        assert named(calls, "anchor_combine_f32") == (points - 1) + (named(calls, "precondition") - 1) + 1, sorted(calls.items())
    else:
        assert named(calls, "store_differences_f32") == 0 and named(calls, "anchor_combine_f32") == 0, calls
    assert named(f64["calls"], "anchor_combine_f32") == 0 and named(f64["calls"], "store_differences_f32") == 0


@pytest.mark.parametrize("case", ["1e-8", "1e-8 max_size_qspace=5"])
@pytest.mark.parametrize("path", [0, 1], ids=["fused", "call_by_call"])
def test_c5_q32_takes_the_f64_solves_iterations(solves, case, path):
    f64, q32 = solves[path][case + "/f64"], solves[path][case + "/q32"]
    solve_criteria(f"C5 {N_C5} at {case}, {'call by call' if path else 'fused'}", f64, q32, 1e-8)
    history_and_ledger(f64, q32, N_C5, case, path)


@pytest.mark.parametrize("case", ["dense 1e-8", "dense 1e-8 max_size_qspace=5"])
@pytest.mark.parametrize("path", [0, 1], ids=["fused", "call_by_call"])
def test_dense_3000_q32_takes_the_f64_solves_iterations(solves, case, path):
    """The criteria of the C5 solves on the dense_3000 matrix (r = H (x - 1), |x*| = 55)."""
    f64, q32 = solves[path][case + "/f64"], solves[path][case + "/q32"]
    solve_criteria(f"dense_3000 at {case[6:]}, {'call by call' if path else 'fused'}", f64, q32, 1e-8, dense_residual)
    history_and_ledger(f64, q32, N_DENSE, case, path)


def test_fused_and_call_by_call_take_the_same_iterations(solves):
    for case in ("1e-8", "1e-8 max_size_qspace=5", "dense 1e-8", "dense 1e-8 max_size_qspace=5"):
        assert solves[0][case + "/q32"]["iterations"] == solves[1][case + "/q32"]["iterations"], case


@pytest.mark.parametrize("case", ["1e-10", "1e-12"])
def test_c5_q32_below_1e_8_is_no_worse_than_the_f64_solve(solves, case):
    """Where the f64 solve converges, the q32 solve's final recomputed residual is at most twice the f64 solve's."""
    f64, q32 = solves[0][case + "/f64"], solves[0][case + "/q32"]
    r64, r32 = c5_residual(f64["x"]), c5_residual(q32["x"])
    print(f"\nC5 {N_C5} at {case}: f64 converged {f64['converged']} in {f64['iterations']} iterations, residual {r64:.3e}; "
          f"q32 converged {q32['converged']} in {q32['iterations']} iterations, residual {r32:.3e}")
    if f64["converged"]:
        assert r32 <= 2 * r64


def test_short_vector_solve_fused_and_call_by_call_agree_bit_for_bit(solves):
    a, b = solves[0]["short/q32"], solves[1]["short/q32"]
    solve_criteria(f"C5 {N_SHORT} at 1e-8 on the short-vector path", solves[0]["short/f64"], a, 1e-8)
    assert a["iterations"] == b["iterations"] and a["errors"] == b["errors"]
    assert np.array_equal(bits(a["x"]), bits(b["x"]))


# ---- 5. the reverse-communication API -----------------------------------------------------------------------------
@pytest.fixture()
def api(ctx):
    import iterative_solver

    iterative_solver.use_context(ctx)
    yield ctx
    iterative_solver.use_context(None)


@pytest.mark.parametrize("n", [20, 50])
def test_rc_diis_quadratic_form_with_q_storage_f32(api, n):
    import device_api_cases as dc
    import iterative_solver
    import rc_problems as rp

    hq = rp.quadratic_matrix(n, 10.0)
    seen = []

    def make():
        s = iterative_solver.NonLinearEquations(n, thresh=1e-8, options="Q_STORAGE=f32,convergence_threshold=1e-8,max_size_qspace=6")
        seen.append(s.q_storage)
        return s

    def loop(s):
        trace, n_iter = rp.loop_quadratic(s, hq, optimize=False)
        x, g = np.zeros(n), np.zeros(n)
        s.solution([0], x, g)
        return trace, n_iter, x, g, s.errors.copy()

    hl, dl, hr, dr = dc.both_routes(make, loop, api)
    dc.assert_same_log(hl, dl)
    assert seen == [4, 4]
    trace, n_iter, x, g, errors = hr
    assert n_iter == dr[1] and 3 < n_iter < 100 and trace[-1][1] == 0  # the loop ended converged
    assert np.all(np.abs(errors) <= 1e-8) and np.linalg.norm(g) <= 1e-8
    np.testing.assert_allclose(x, 1.0, rtol=0, atol=1e-8)
    assert np.array_equal(dc.bits(x), dc.bits(dr[2]))
    f64 = iterative_solver.NonLinearEquations(n, thresh=1e-8, options="convergence_threshold=1e-8,max_size_qspace=6")
    try:
        assert f64.q_storage == 8
        _, n_f64 = rp.loop_quadratic(f64, hq, optimize=False)
    finally:
        f64.finalize()
    assert n_iter <= n_f64 + 1, (n_iter, n_f64)


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------
def test_rc_refusals_name_their_option_and_the_family(api):
    import iterative_solver

    for options, words, kw in (("Q_STORAGE=f32,Q_REFINE=1", ("Q_REFINE", "NonLinearEquations"), {}),
                               ("Q_REFINE=1", ("Q_REFINE", "NonLinearEquations"), {}),
                               ("Q_STORAGE=f32", ("Q_STORAGE=f32", "NonLinearEquations", "DIIS"), dict(algorithm="BFGS"))):
        with pytest.raises(RuntimeError) as e:
            iterative_solver.NonLinearEquations(8, options=options, **kw).finalize()
        assert all(w in str(e.value) for w in words), (options, str(e.value))
    for family, make in (("Optimize", lambda: iterative_solver.Optimize(8, options="Q_STORAGE=f32")),):
        with pytest.raises(RuntimeError) as e:
            make().finalize()
        assert "Q_STORAGE=f32" in str(e.value) and family in str(e.value)
    s = iterative_solver.NonLinearEquations(8, options="Q_STORAGE=f32", algorithm="DIIS")
    assert s.q_storage == 4
    s.finalize()


def test_use_context_after_a_refused_initialize_does_not_report_its_error(ctx):
    """IterativeSolverHbmSetContext cannot fail: it does not leave the error of the call before it standing."""
    import iterative_solver

    iterative_solver.use_context(ctx)
    try:
        with pytest.raises(RuntimeError, match="Q_REFINE"):
            iterative_solver.NonLinearEquations(8, options="Q_REFINE=1").finalize()
    finally:
        iterative_solver.use_context(None)


class TwoRanks:
    """A host communicator that says it is rank 0 of 2 (no peer: the refusals come before any exchange)."""

    nranks, rank = 2, 0

    def __init__(self):
        import subspace_hip as sh

        self.allreduce_cb = sh.ALLREDUCE_FN(lambda buf, n, user: 0)
        self.allgather_cb = sh.ALLGATHER_FN(self._allgather)

    @staticmethod
    def _allgather(send, recv, nbytes, user):
        for r in range(2):
            C.memmove(recv + r * nbytes, send, nbytes)
        return 0


def test_more_than_one_rank_is_refused(ctx):
    import iterative_solver
    import itsolv_hbm as ih
    import subspace_hip as sh

    with sh.Context(0) as two:
        two.attach_host_comm(TwoRanks())
        with pytest.raises(RuntimeError, match="more than one rank"):
            ih.diis_synthetic(two, 64, **ih.c5_spec(64), q32=True)
        iterative_solver.use_context(two)
        try:
            with pytest.raises(RuntimeError) as e:
                iterative_solver.NonLinearEquations(64, options="Q_STORAGE=f32").finalize()
            assert all(w in str(e.value) for w in ("Q_STORAGE=f32", "NonLinearEquations", "more than one rank")), str(e.value)
        finally:
            iterative_solver.use_context(None)


def test_a_p_space_is_refused(ctx):
    import itsolv_hbm as ih

    with pytest.raises(RuntimeError, match="P space"):
        ih.diis_synthetic(ctx, 64, **ih.c5_spec(64), q32=True, max_p=4)
    assert ih.diis_synthetic(ctx, 64, **ih.c5_spec(64), q32=True)["converged"]  # without the option it runs
