"""The fused solver passes over an f32 Q space beside f64 R vectors (include/subspace_hip.h ssp_q32_*):
the inner product whose column list mixes f64 and f32 vectors, the P-aware updates with f32 dense
sources, and the q32 Davidson solve that runs on them.  The mixed-precision rule of test_mixed_gpu.py
applies per column / per source: expected values come from the library's own f64 entry points on widened
copies (bit-identical on the exact path and for the updates), reductions on the bandwidth path are held
to the project's reduction bound against the exact sum of the rounded products.

As in test_mixed_gpu.py every kernel test runs with exact_max = 0 (the bandwidth kernels at every size)
and at the default 2048 (sizes up to 2048 only).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_mixed_gpu import (EPS, EPS32, EXACT_MAX_DEFAULT, F32, F64, Pool, exact_sums, values,  # noqa: F401
                            exact_max, pool, with_modes)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in cast")]

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "iterative-solver_amd")

# (rows; f64 columns, f32 columns)
MIXES = [(1, 1, 1), (3, 2, 3), (8, 5, 7), (8, 16, 112), (17, 3, 66), (4, 0, 9), (4, 9, 0)]


def interleaved(n64, n32):
    """Column dtypes with the two kinds interleaved evenly, not sorted (and not f64 first)."""
    k = n64 + n32
    return [F64 if (j + 1) * n64 // k > j * n64 // k else F32 for j in range(k)]


def bound_check(got, x, y, xs, ys):
    ref, mag, slack = exact_sums([s * v for s, v in zip(xs, x)], [s * v for s, v in zip(ys, y)])
    assert np.all(np.abs(got - ref) <= (64 * EPS - slack) * mag + 1e-300), np.max(np.abs(got - ref) / (mag + 1e-300))


# ---- 1. gemm_inner_cols -----------------------------------------------------------------------------
@pytest.mark.parametrize("m,n64,n32", MIXES, ids=[f"{m}-{a}-{b}" for m, a, b in MIXES])
@with_modes([0, 1, 5, 63, 64, 65, 1003, 100_003])
def test_gemm_inner_cols_values(ctx, pool, exact_max, n, m, n64, n32):
    r = np.random.default_rng(1000 * m + 10 * n64 + n32 + n % 89)
    dts = interleaved(n64, n32)
    k = len(dts)
    xs, ys = r.uniform(0.5, 2, m), r.uniform(0.5, 2, k)
    x = [values(r, n, F64) for _ in range(m)]
    y = [values(r, n, dt) for dt in dts]
    dx, dy = [pool.up(v) for v in x], [pool.up(v, dt) for v, dt in zip(y, dts)]
    got = ctx.q32_gemm_inner_cols(dx, dy, xs=xs, ys=ys)
    assert got.shape == (m, k)
    assert np.array_equal(got, ctx.q32_gemm_inner_cols(dx, dy, xs=xs, ys=ys))  # the same bits again
    if n == 0:
        assert not got.any()
    elif exact_max:
        dyw = [v if dt == F64 else pool.up(w) for v, w, dt in zip(dy, y, dts)]
        assert np.array_equal(got, ctx.gemm_inner_scaled(dx, xs, dyw, ys))
    else:
        bound_check(got, x, y, xs, ys)
    for v, w, dt in zip(dy, y, dts):  # the columns are untouched
        assert np.array_equal(v.numpy(), w.astype(dt))


@pytest.mark.parametrize("pattern", ["alternating", "groups_of_5"])
def test_gemm_inner_cols_exact_integers(ctx, pool, pattern):
    """Small integers (exact in f32 and f64): catches row, column, group and quad mix-ups."""
    ctx.set_exact_max(0)
    try:
        n = 4096 + 24 + 3
        xs = [np.full(n, float(i + 1)) for i in range(8)]
        ys = [np.arange(n, dtype=float) % 7 * (j + 1) for j in range(48)]
        dts = [(F32 if j % 2 else F64) if pattern == "alternating" else (F32 if (j // 5) % 2 else F64) for j in range(48)]
        ref = np.array([[np.dot(a, b) for b in ys] for a in xs])
        dx, dy = [pool.up(v) for v in xs], [pool.up(v, dt) for v, dt in zip(ys, dts)]
        assert np.array_equal(ctx.q32_gemm_inner_cols(dx, dy), ref)
    finally:
        ctx.set_exact_max(EXACT_MAX_DEFAULT)


def test_gemm_inner_cols_forwards_one_type_columns(ctx, pool):
    n = 100_003
    r = np.random.default_rng(31)
    xs, ys = r.uniform(0.5, 2, 3), r.uniform(0.5, 2, 9)
    x = [values(r, n, F64) for _ in range(3)]
    y = [values(r, n, F32) for _ in range(9)]
    dx, d64, d32 = [pool.up(v) for v in x], [pool.up(v) for v in y], [pool.up(v, F32) for v in y]
    assert np.array_equal(ctx.q32_gemm_inner_cols(dx, d64, xs=xs, ys=ys), ctx.gemm_inner_scaled(dx, xs, d64, ys))
    assert np.array_equal(ctx.q32_gemm_inner_cols(dx, d32, xs=xs, ys=ys), ctx.mx_gemm_inner(dx, d32, xs=xs, ys=ys))


@pytest.mark.parametrize("n", [100_003, 0], ids=["n100003", "empty_shard"])
def test_gemm_inner_cols_with_a_communicator(n):
    """The reduction path of a sharded solve (results left on the device, exchanged, then published) in a
    context of its own with a one-rank peer-memory communicator; an empty shard delivers zeros through
    the same exchange."""
    import subspace_hip as sh

    m, n64, n32 = 8, 16, 112
    r = np.random.default_rng(77)
    dts = interleaved(n64, n32)
    xs, ys = r.uniform(0.5, 2, m), r.uniform(0.5, 2, len(dts))
    x = [values(r, n, F64) for _ in range(m)]
    y = [values(r, n, dt) for dt in dts]
    with sh.Context(0) as c:
        c.attach_p2p(1, 0, sh.Context.p2p_unique_id())
        c.set_exact_max(0)
        p = Pool(c)
        dx, dy = [p.up(v) for v in x], [p.up(v, dt) for v, dt in zip(y, dts)]
        got = c.q32_gemm_inner_cols(dx, dy, xs=xs, ys=ys)
        again = c.q32_gemm_inner_cols(dx, dy, xs=xs, ys=ys)
        p.free()
    assert got.shape == (m, n64 + n32) and np.array_equal(got, again)
    if n == 0:
        assert not got.any()
    else:
        bound_check(got, x, y, xs, ys)


# ---- 2. the updates ---------------------------------------------------------------------------------
def p_vectors(r, kp, n, offset):
    """kp sparse vectors of 1-12 entries (global indices) with repeated and shared indices: the shard's
    first and last element, the n mod 4 tail, and indices outside [offset, offset + n)."""
    special = [offset, offset + n - 1] + [offset + n - 1 - t for t in range(n % 4)]
    outside = [offset + n, offset + n + 7] + ([offset - 1] if offset else [])
    ps = []
    for i in range(kp):
        cnt = int(r.integers(1, 13))
        idx = [int(offset + r.integers(0, n)) for _ in range(cnt)]
        idx[0] = special[i % len(special)]  # shared between the P vectors
        if cnt > 2:
            idx[1] = outside[i % len(outside)]
        if cnt > 3:
            idx[2] = special[(i + 1) % len(special)]
        ps.append({j: float(r.uniform(-1, 1)) for j in idx})
    return ps


UPDATE_SHAPES = [(0, 3, 2), (4, 48, 8), (16, 65, 3), (5, 0, 4), (3, 7, 16)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "ys"])
@pytest.mark.parametrize("kp,k,m", UPDATE_SHAPES, ids=[f"{a}-{b}-{c}" for a, b, c in UPDATE_SHAPES])
@with_modes([1, 5, 1003, 100_003])
def test_updates_equal_the_f64_entry_points_on_widened_sources(ctx, pool, exact_max, n, kp, k, m, scaled):
    r = np.random.default_rng(10_000 * kp + 100 * k + m + n % 97)
    offset = 12_345
    ps = p_vectors(r, kp, n, offset)
    pa, al = r.uniform(-1, 1, (kp, m)), r.uniform(-1, 1, (k, m))
    ys = r.uniform(0.5, 2, m) if scaled else None
    x = [values(r, n, F32) for _ in range(k)]
    y0 = [values(r, n, F64) for _ in range(m)]
    dx, dxw = [pool.up(v, F32) for v in x], [pool.up(v) for v in x]
    # block update
    got, ref = [pool.up(v) for v in y0], [pool.up(v) for v in y0]
    ctx.q32_block_update(pa, ps, al, dx, got, ys, offset=offset)
    ctx.block_update(pa, ps, al, dxw, None, ref, ys, offset=offset)
    for j in range(m):
        assert np.array_equal(got[j].numpy(), ref[j].numpy()), ("block_update", j)
    # construct_solution, with a deferred zero fill pending on one destination and garbage in the others
    got, ref = [pool.up(np.full(n, 9.0)) for _ in range(m)], [pool.up(np.full(n, 7.0)) for _ in range(m)]
    ctx.fill(0.0, got[0])
    ctx.q32_construct_solution(pa, ps, al, dx, got, offset=offset)
    ctx.construct_solution(pa, ps, al, dxw, ref, offset=offset)
    for j in range(m):
        assert np.array_equal(got[j].numpy(), ref[j].numpy()), ("construct_solution", j)
    ctx.synchronize()
    assert np.array_equal(got[0].numpy(), ref[0].numpy())  # the pending fill did not resurface
    for v, w in zip(dx, x):
        assert np.array_equal(v.numpy(), w.astype(F32))  # the sources are untouched


# ---- 3. ledger, argument errors ---------------------------------------------------------------------
def test_ledger_counts_storage_bytes(ctx, pool):
    ctx.set_exact_max(0)
    try:
        n = 100_000
        rows = [pool.up(np.ones(n)) for _ in range(3)]
        c64, c32 = [pool.up(np.ones(n)) for _ in range(2)], [pool.up(np.ones(n), F32) for _ in range(5)]
        cols = [c32[0], c64[0], c32[1], c32[2], c64[1], c32[3], c32[4]]
        y = [pool.up(np.ones(n)) for _ in range(2)]
        ctx.ledger_reset()
        ctx.ledger_enable(True)
        ctx.q32_gemm_inner_cols(rows, cols)
        ctx.q32_block_update(np.zeros((0, 2)), [], np.ones((5, 2)), c32, y)
        ctx.q32_construct_solution(np.zeros((0, 2)), [], np.ones((5, 2)), c32, y)
        ctx.synchronize()
        led = ctx.ledger()
        ctx.ledger_enable(False)
        assert led["gemm_inner_cols"]["calls"] == 1
        assert led["gemm_inner_cols"]["bytes"] == n * (8 * 3 + 8 * 2 + 4 * 5)
        assert led["gemm_outer_f32"]["calls"] == 2
        assert led["gemm_outer_f32"]["bytes"] == n * (4 * 5 + 16 * 2) + n * (4 * 5 + 8 * 2)
    finally:
        ctx.ledger_enable(False)
        ctx.set_exact_max(EXACT_MAX_DEFAULT)


def test_argument_errors(ctx, pool):
    import ctypes as C

    import subspace_hip as sh

    x, q, y = pool.up(np.ones(8)), pool.up(np.ones(8), F32), pool.up(np.ones(8))
    lib, out = ctx.lib, np.zeros(4)
    od = out.ctypes.data_as(sh.PD)

    def cols(ptrs, tys, m=1, k=None, n=8, rows=None):
        k = len(ptrs) if k is None else k
        rp = (C.c_void_p * 1)(x.ptr if rows is None else rows)
        cp = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        ty = (C.c_int * max(1, len(tys)))(*tys)
        return lib.ssp_q32_gemm_inner_cols(ctx.handle, rp, None, m, cp, ty, None, k, n, od)

    assert cols([q.ptr, y.ptr], [1, 0]) == 0
    assert cols([q.ptr, y.ptr], [1, 2]) == 3  # bad dtype
    assert cols([q.ptr, None], [1, 0]) == 3  # null column
    assert cols([q.ptr + 4, y.ptr], [1, 0], n=4) == 3  # misaligned column
    assert cols([q.ptr, y.ptr], [1, 0], rows=x.ptr + 8, n=4) == 3  # misaligned row
    assert cols([q.ptr, y.ptr], [1, 0], m=-1) == 3
    assert cols([q.ptr, y.ptr], [1, 0], k=-1) == 3
    one = np.ones(1)
    ptr = np.zeros(1, dtype=np.uint64)

    def update(f, src, dst, k=1, m=1, n=8, extra=()):
        sp, dp = (C.c_void_p * 1)(src), (C.c_void_p * 1)(dst)
        return f(ctx.handle, None, sh._zptr(ptr), None, None, 0, sh._dptr(one), sp, k, dp, *extra, m, n, 0)

    for f, extra in ((lib.ssp_q32_construct_solution, ()), (lib.ssp_q32_block_update, (None,))):
        assert update(f, q.ptr, y.ptr, extra=extra) == 0
        assert update(f, None, y.ptr, extra=extra) == 3
        assert update(f, q.ptr + 4, y.ptr, n=4, extra=extra) == 3
        assert update(f, q.ptr, None, extra=extra) == 3
        assert update(f, q.ptr, y.ptr, k=-1, extra=extra) == 3
        assert update(f, q.ptr, y.ptr, m=-1, extra=extra) == 3
    with pytest.raises(TypeError):
        ctx.q32_block_update(np.zeros((0, 1)), [], np.ones((1, 1)), [x], [y])  # an f64 source
    with pytest.raises(TypeError):
        ctx.q32_gemm_inner_cols([q], [y])  # an f32 row


# ---- 4. the q32 Davidson solve on the fused passes ----------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import itsolv_hbm as ih
import subspace_hip as sh
max_p = int(sys.argv[2])
REDUCING = ("dot", "gemm_inner", "axpy_inner", "scal_inner", "axpy_norm", "axpy_gram", "axpy_pairs_norm", "select",
            "gemm_inner_sparse", "gemm_inner_f32", "dot_f32", "gemm_inner_cols")
kw = dict(nroots=4, convergence_threshold=1e-6, max_size_qspace=24, reset_D=8)
if max_p:
    kw["max_p"] = max_p
out = {}
with sh.Context(0) as ctx:
    for name, q32 in (("f64", False), ("q32", True)):
        ctx.ledger_reset()
        ctx.ledger_enable(True)
        r = ih.davidson_synthetic(ctx, 100_003, 0.1, 2, 20251015, q32=q32, **kw)
        ctx.synchronize()
        ctx.ledger_enable(False)
        led = ctx.ledger()
        calls = {op: v["calls"] for op, v in led.items()}
        out[name] = {"converged": bool(r["converged"]), "iterations": int(r["iterations"]),
                     "eigenvalues": [float(e) for e in r["eigenvalues"]],
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
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module", params=[0, 8], ids=["no_p", "max_p8"])
def solves(request):
    """(fused, call by call) of one problem: each child runs the f64 and the q32 solve."""
    return solve(request.param, 0), solve(request.param, 10**15)


def q32_criteria(run):
    """The criteria of test_mixed_gpu.test_davidson_synthetic_with_f32_q_space."""
    n, rho, rank = 100_003, 0.1, 2
    f64, q32 = run["f64"], run["q32"]
    norm2 = 1.0 + n + rank * rho * n
    diff = max(abs(a - b) for a, b in zip(q32["eigenvalues"], f64["eigenvalues"]))
    print(f"\niterations f64 {f64['iterations']} q32 {q32['iterations']}, max eigenvalue difference {diff:.3e} "
          f"(bound {4 * EPS32 * norm2:.3e})")
    assert f64["converged"] and q32["converged"]
    assert diff <= 4 * EPS32 * norm2
    assert q32["iterations"] <= f64["iterations"] + 3


def test_q32_solve_on_the_fused_passes(solves):
    q32_criteria(solves[0])
    calls = solves[0]["q32"]["calls"]
    assert calls.get("gemm_inner_cols", 0) > 0, calls  # the batched rows ran on the mixed inner product
    # the updates ran as one pass each (hbm_handlers_f32.h fused_block_update / fused_construct_solution for
    # VecF32), not as gemm_outer(P) + gemm_outer(Q, D) behind a pass that stores the pending scale: with a
    # P space their fix-ups show in the ledger and no sparse gemm_outer does, and the q32 solve stores no
    # more scales than the f64 solve
    f64_calls = solves[0]["f64"]["calls"]
    assert calls.get("gemm_outer_sparse", 0) == 0, calls
    assert calls.get("scal", 0) <= f64_calls.get("scal", 0), (calls, f64_calls)
    if "p_action(synthetic)" in calls:
        assert calls.get("block_update_sparse", 0) > 0 and calls.get("construct_solution_sparse", 0) > 0, calls
        assert calls["block_update_sparse"] == f64_calls["block_update_sparse"], (calls, f64_calls)
        assert calls["construct_solution_sparse"] == f64_calls["construct_solution_sparse"], (calls, f64_calls)


def test_q32_solve_call_by_call(solves):
    q32_criteria(solves[1])


def test_q32_solve_makes_no_more_reductions_than_the_f64_solve(solves):
    """Reducing calls (each a host round trip) per iteration, ledger on: with the batched overlap rows,
    the one-pass block update and construct_solution, the q32 solve makes the f64 solve's count."""
    f64, q32 = solves[0]["f64"], solves[0]["q32"]
    per64, per32 = f64["reducing"] / f64["iterations"], q32["reducing"] / q32["iterations"]
    print(f"\nreducing calls per iteration: f64 {per64:.2f} ({f64['reducing']} / {f64['iterations']}), "
          f"q32 {per32:.2f} ({q32['reducing']} / {q32['iterations']})\nq32 calls {q32['calls']}\nf64 calls {f64['calls']}")
    assert per32 <= per64
