"""Mixed precision (include/subspace_hip.h ssp_mx_*, *_f32): vectors stored in binary32, arithmetic in
FP64.  One rule is tested throughout: an f32 operand is widened as it is loaded, the operation is the
f64 entry point's on the widened values, and an f32 destination is the f64 result rounded once.  So the
expected values come from the library's own f64 entry points run on widened copies of the same data
(bit-identical for f64 destinations, `.astype(float32)` of it for f32 destinations); reductions are
held to the project's reduction bound against the exact sum of the rounded products.

Every kernel test runs with exact_max = 0 (the bandwidth kernels at every size) and at the default
2048 (the short-vector path; sizes up to 2048 only, longer vectors take the same kernels as before).
"""
import math

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered in cast")]
EPS = np.finfo(np.float64).eps
EPS32 = float(np.finfo(np.float32).eps)
EXACT_MAX_DEFAULT = 2048  # ssp_ctx_set_exact_max default (include/subspace_hip.h)
F32, F64 = np.float32, np.float64
PAIRS = [(F32, F64), (F64, F32), (F32, F32)]  # (dtype of x / xx, dtype of y / yy)


def modes(sizes):
    """(exact_max, n): every size on the bandwidth kernels, the sizes of the exact path on it."""
    return [(0, n) for n in sizes] + [(EXACT_MAX_DEFAULT, n) for n in sizes if 0 < n <= EXACT_MAX_DEFAULT]


@pytest.fixture
def exact_max(ctx, request):
    ctx.set_exact_max(request.param)
    yield request.param
    ctx.set_exact_max(EXACT_MAX_DEFAULT)


def with_modes(sizes):
    return pytest.mark.parametrize("exact_max,n", modes(sizes), indirect=["exact_max"],
                                   ids=[f"{'exact' if e else 'bw'}-{n}" for e, n in modes(sizes)])


def red_tol(terms):
    return 64 * EPS * np.sum(np.abs(terms)) + 1e-300


def values(r, n, dt):
    """uniform(-1, 1), rounded to f32 for an f32 operand; returned widened (float64 array)."""
    a = r.uniform(-1, 1, n)
    return a.astype(F32).astype(F64) if dt == F32 else a


class Pool:
    """Device vectors of a test, freed at its end."""

    def __init__(self, ctx):
        self.ctx, self.vs = ctx, []

    def up(self, a, dt=F64):
        v = self.ctx.upload(a, dt)
        self.vs.append(v)
        return v

    def free(self):
        for v in self.vs:
            v.free()


@pytest.fixture
def pool(ctx):
    p = Pool(ctx)
    yield p
    p.free()


# ---- 1. storage ---------------------------------------------------------------------------------
def test_storage_takes_four_bytes_per_element(ctx):
    ctx.release_cached()
    n = 1 << 20
    base = ctx.memory_stats()[0]
    v32 = ctx.alloc(n, F32)
    assert v32.dtype == F32
    assert ctx.memory_stats()[0] - base == 4 << 20
    v64 = ctx.alloc(n)
    assert v64.dtype == F64
    assert ctx.memory_stats()[0] - base == (4 << 20) + (8 << 20)
    v32.free()
    v64.free()
    assert ctx.memory_stats()[0] == base


@pytest.mark.parametrize("n", [0, 1, 3, 1003, (1 << 20) + 5])
def test_upload_download_round_trip_is_bit_exact(ctx, n):
    a = np.random.default_rng(n).standard_normal(n).astype(F32)
    if n > 3:
        a[:4] = [np.float32(-0.0), np.float32(np.inf), np.finfo(F32).tiny / 4, np.finfo(F32).max]
    v = ctx.upload(a, F32)
    got = v.numpy()
    assert got.dtype == F32
    assert np.array_equal(got.view(np.uint32), a.view(np.uint32))
    w = ctx.alloc(n, F32)
    ctx.upload_into(w, a)
    assert np.array_equal(ctx.download(w).view(np.uint32), a.view(np.uint32))
    v.free()
    w.free()


# ---- 2. convert known answers ---------------------------------------------------------------------
@with_modes([7])
def test_convert_rounds_to_nearest_even(ctx, pool, exact_max, n):
    y = np.array([1 + 2.0**-24, 1 + 3 * 2.0**-24, 1 + 2.0**-24 + 2.0**-50, -0.0, 1e39, -1e39, 0.1])
    want = np.array([1.0, 1 + 2.0**-22, 1 + 2.0**-23, -0.0, np.inf, -np.inf, float(np.float32(0.1))])
    d64, d32, back = pool.up(y), pool.up(np.zeros(n), F32), pool.up(np.zeros(n))
    ctx.mx_copy(d32, d64)
    ctx.mx_copy(back, d32)
    got = back.numpy()
    assert np.array_equal(got, want)
    assert np.signbit(got[3])
    assert np.array_equal(d32.numpy().view(np.uint32), y.astype(F32).view(np.uint32))
    # with a scale the product is rounded to f64 first, then to f32
    z = np.array([1 + 2.0**-24, 0.3, -0.7, 1e-30, 3.0, 1e38, 1 / 3])
    dz = pool.up(z)
    ctx.mx_copy(d32, dz, ys=3.5)
    assert np.array_equal(d32.numpy().view(np.uint32), (3.5 * z).astype(F32).view(np.uint32))


# ---- 3. elementwise ops ---------------------------------------------------------------------------
ELEMENTWISE_SIZES = [0, 1, 2, 3, 4, 5, 7, 64, 255, 256, 257, 1003, 100_003, (1 << 20) + 5]


@with_modes(ELEMENTWISE_SIZES)
def test_copy_and_axpy_equal_the_f64_entry_points_on_widened_operands(ctx, pool, exact_max, n):
    r = np.random.default_rng(n + 17)
    for tx, ty in PAIRS:
        # copy, x (tx) = ys * y (ty)
        y = values(r, n, ty)
        dy, dyw = pool.up(y, ty), pool.up(y)
        for ys in (1.0, 3.5):
            dx, ref = pool.up(np.full(n, 9.0), tx), pool.up(np.full(n, 9.0))
            ctx.mx_copy(dx, dy, ys=ys)
            ctx.scal_copy(ys, ref, dyw) if ys != 1.0 else ctx.copy(ref, dyw)
            want = ref.numpy()
            assert np.array_equal(want, ys * y)
            got = dx.numpy()
            assert got.dtype == tx
            assert np.array_equal(got, want.astype(tx)), (tx, ty, ys)
        # axpy, y (ty) = fma(alpha, x (tx), y)
        x, y0 = values(r, n, tx), values(r, n, ty)
        dx, dy = pool.up(x, tx), pool.up(y0, ty)
        dxw, dyw = pool.up(x), pool.up(y0)
        ctx.mx_axpy(-0.75, dx, dy)
        ctx.axpy(-0.75, dxw, dyw)
        assert np.array_equal(dy.numpy(), dyw.numpy().astype(ty)), (tx, ty)
        assert np.array_equal(dx.numpy(), x.astype(tx))  # the source is untouched


@with_modes(ELEMENTWISE_SIZES)
def test_fill_and_scal_dispatch_on_the_vector_dtype(ctx, pool, exact_max, n):
    r = np.random.default_rng(n + 29)
    x = values(r, n, F32)
    dx, dxw = pool.up(x, F32), pool.up(x)
    ctx.scal(3.3, dx)
    ctx.scal(3.3, dxw)
    assert np.array_equal(dxw.numpy(), 3.3 * x)
    assert np.array_equal(dx.numpy().view(np.uint32), dxw.numpy().astype(F32).view(np.uint32))
    for alpha in (0.1, 0.0, -0.0, 1e39):
        ctx.fill(alpha, dx)
        assert np.array_equal(dx.numpy().view(np.uint32), np.full(n, alpha).astype(F32).view(np.uint32)), alpha


def test_f32_fill_is_stored_behind_a_deferred_f64_fill(ctx, pool):
    """A deferred f64 zero fill is stored before a mixed call reads the vector."""
    n = 100_003
    y = values(np.random.default_rng(5), n, F64)
    d64, d32 = pool.up(y), pool.up(np.ones(n), F32)
    ctx.fill(0.0, d64)  # deferred (n > exact_max)
    ctx.mx_axpy(2.0, d64, d32)
    assert np.array_equal(d32.numpy(), np.ones(n, dtype=F32))
    ctx.mx_copy(d32, d64)
    assert not d32.numpy().any()


# ---- 4. gemm_outer --------------------------------------------------------------------------------
def outer_reference(ctx, pool, al, xw, y0, xs, set_, k0=0, k1=None):
    """The f64 entry point on widened sources: f64 result vectors."""
    k1 = len(xw) if k1 is None else k1
    dy = [pool.up(v) for v in y0]
    if set_:
        ctx.gemm_outer_set_scaled(al[k0:k1], xw[k0:k1], None if xs is None else xs[k0:k1], dy)
    else:
        ctx.gemm_outer_scaled(al[k0:k1], xw[k0:k1], None if xs is None else xs[k0:k1], dy, None)
    return [v.numpy() for v in dy]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "xs"])
@pytest.mark.parametrize("set_", [False, True], ids=["rmw", "set"])
@pytest.mark.parametrize("k,m", [(1, 1), (3, 5), (48, 8), (5, 16), (7, 17), (65, 3)])
@with_modes([1, 5, 1003, 100_003])
def test_gemm_outer_equals_the_f64_entry_point_on_widened_sources(ctx, pool, exact_max, n, k, m, set_, scaled):
    r = np.random.default_rng(1000 * k + 10 * m + n % 97)
    al = r.uniform(-1, 1, (k, m))
    xs = r.uniform(0.5, 2.0, k) if scaled else None
    for tx, ty in PAIRS:
        x = [values(r, n, tx) for _ in range(k)]
        y0 = [values(r, n, ty) for _ in range(m)]
        dx = [pool.up(v, tx) for v in x]
        dxw = dx if tx == F64 else [pool.up(v) for v in x]
        dy = [pool.up(v, ty) for v in y0]
        ctx.mx_gemm_outer(al, dx, dy, xs=xs, set=set_)
        got = [v.numpy() for v in dy]
        if ty == F32 and k > 64 and not exact_max:
            # f32 destinations on the bandwidth kernels: one launch per 64 sources, each a read-modify-
            # write of the f32 destinations (the rounding rule of include/subspace_hip.h)
            part = [v.astype(F32).astype(F64) for v in outer_reference(ctx, pool, al, dxw, y0, xs, set_, 0, 64)]
            ref = outer_reference(ctx, pool, al, dxw, part, xs, False, 64, k)
        else:
            ref = outer_reference(ctx, pool, al, dxw, y0, xs, set_)
        for j in range(m):
            assert got[j].dtype == ty
            assert np.array_equal(got[j], ref[j].astype(ty)), (tx, ty, j)
        for i in range(k):
            assert np.array_equal(dx[i].numpy(), x[i].astype(tx))
        pool.free()
        pool.vs = []


@pytest.mark.parametrize("k,m", [(48, 8), (7, 17), (65, 3), (9, 1)])
@with_modes([1003, 4099])
def test_gemm_outer_exact_integers(ctx, pool, exact_max, n, k, m):
    """Small integers (exact in f32 and f64) with a distinct alpha per (i, j): catches index mix-ups
    between sources, destinations and the elements of a quad."""
    e = np.arange(n)
    x = [((e * (i + 3)) % 7 - 3).astype(F64) for i in range(k)]
    al = (np.arange(k * m).reshape(k, m) % 13 + 1).astype(F64) * np.where(np.arange(k * m).reshape(k, m) % 2, -1, 1)
    y0 = [((e + j) % 5).astype(F64) for j in range(m)]
    for tx, ty in PAIRS:
        for set_ in (False, True):
            dx = [pool.up(v, tx) for v in x]
            dy = [pool.up(v, ty) for v in y0]
            ctx.mx_gemm_outer(al, dx, dy, set=set_)
            for j in range(m):
                want = sum(al[i, j] * x[i] for i in range(k)) + (0 if set_ else y0[j])
                assert np.abs(want).max() < 2**24
                assert np.array_equal(dy[j].numpy(), want.astype(ty)), (tx, ty, set_, j)
            pool.free()
            pool.vs = []


def test_gemm_outer_rejects_bad_arguments(ctx, pool):
    import subspace_hip as sh

    x, y = pool.up(np.ones(8), F32), pool.up(np.ones(8))
    with pytest.raises(sh.SspError) as e:
        ctx.mx_gemm_outer(np.ones((1, 1)), [x], [x])  # a destination aliases a source
    assert e.value.code == 3
    lib = ctx.lib
    out = np.zeros(1)
    assert lib.ssp_mx_dot(ctx.handle, x.ptr, 2, y.ptr, 0, 8, out.ctypes.data_as(sh.PD)) == 3  # bad enum
    assert lib.ssp_mx_dot(ctx.handle, x.ptr + 4, 1, y.ptr, 0, 4, out.ctypes.data_as(sh.PD)) == 3  # misaligned
    assert lib.ssp_mx_copy(ctx.handle, None, 1, y.ptr, 0, 1.0, 8) == 3  # null
    with pytest.raises(TypeError):
        ctx.mx_gemm_inner([x, y], [y])  # one side, two dtypes


# ---- 5. gemm_inner and dot ------------------------------------------------------------------------
LD_EPS = float(np.finfo(np.longdouble).eps)


def exact_sums(xw, yw):
    """(sums, sums of |terms|) of the rounded f64 products of every pair.  Short vectors: math.fsum.
    Long ones: pairwise sums in 80-bit extended precision, whose error (at most 64 * 2^-64 of the sum of
    |terms| for these lengths) is taken off the tolerance by the caller through `slack`."""
    m, k = len(xw), len(yw)
    s, a = np.zeros((m, k)), np.zeros((m, k))
    n = len(xw[0]) if m else 0
    fsum = n <= 2048 or LD_EPS > 2e-19
    for i in range(m):
        for j in range(k):
            t = xw[i] * yw[j]
            s[i, j] = math.fsum(t) if fsum else float(np.sum(t.astype(np.longdouble)))
            a[i, j] = np.sum(np.abs(t))
    slack = 0.0 if fsum else 64 * 2.0**-64
    return s, a, slack


@pytest.mark.parametrize("m,k", [(8, 48), (48, 8), (1, 1), (3, 3), (16, 64), (17, 65)])
@with_modes([0, 1, 5, 1003, 100_003])
def test_gemm_inner_and_dot(ctx, pool, exact_max, n, m, k):
    r = np.random.default_rng(100 * m + k + n % 89)
    for tx, ty in PAIRS:
        x = [values(r, n, tx) for _ in range(m)]
        y = [values(r, n, ty) for _ in range(k)]
        dx, dy = [pool.up(v, tx) for v in x], [pool.up(v, ty) for v in y]
        got = ctx.mx_gemm_inner(dx, dy)
        assert got.shape == (m, k)
        assert np.array_equal(got, ctx.mx_gemm_inner(dx, dy))  # bitwise reproducible
        dxw = dx if tx == F64 else [pool.up(v) for v in x]
        dyw = dy if ty == F64 else [pool.up(v) for v in y]
        if exact_max:
            assert np.array_equal(got, ctx.gemm_inner(dxw, dyw)), (tx, ty)
        else:
            ref, mag, slack = exact_sums(x, y)
            assert np.all(np.abs(got - ref) <= (64 * EPS - slack) * mag + 1e-300), (tx, ty)
        if (m, k) in ((1, 1), (3, 3)):
            d = ctx.mx_dot(dx[0], dy[0])
            assert d == ctx.mx_dot(dx[0], dy[0])
            if exact_max:
                assert d == ctx.dot(dxw[0], dyw[0])
            else:
                t = x[0] * y[0]
                assert abs(d - math.fsum(t)) <= red_tol(t)
        pool.free()
        pool.vs = []


@with_modes([1003, 100_003])
def test_gemm_inner_scales_apply_on_load(ctx, pool, exact_max, n):
    r = np.random.default_rng(n)
    m, k = 3, 9
    xs, ys = r.uniform(0.5, 2, m), r.uniform(0.5, 2, k)
    for tx, ty in PAIRS:
        x = [values(r, n, tx) for _ in range(m)]
        y = [values(r, n, ty) for _ in range(k)]
        dx, dy = [pool.up(v, tx) for v in x], [pool.up(v, ty) for v in y]
        got = ctx.mx_gemm_inner(dx, dy, xs=xs, ys=ys)
        if exact_max:
            dxw, dyw = [pool.up(v) for v in x], [pool.up(v) for v in y]
            assert np.array_equal(got, ctx.gemm_inner_scaled(dxw, xs, dyw, ys))
        else:
            ref, mag, slack = exact_sums([s * v for s, v in zip(xs, x)], [s * v for s, v in zip(ys, y)])
            assert np.all(np.abs(got - ref) <= (64 * EPS - slack) * mag + 1e-300), (tx, ty)
        pool.free()
        pool.vs = []


@pytest.mark.parametrize("tx,ty", PAIRS)
def test_gemm_inner_asymmetric_layout_one_side_f32(ctx, pool, tx, ty):
    """The integer case of test_ops_gpu.test_gemm_inner_asymmetric_layout: catches row / column swaps
    in the MFMA accumulator mapping and misplaced elements of a quad."""
    ctx.set_exact_max(0)
    try:
        n = 4096 + 24 + 3
        xs = [np.full(n, float(i + 1)) for i in range(8)]
        ys = [np.arange(n, dtype=float) % 7 * (j + 1) for j in range(48)]
        ref = np.array([[np.dot(a, b) for b in ys] for a in xs])
        dx, dy = [pool.up(v, tx) for v in xs], [pool.up(v, ty) for v in ys]
        assert np.array_equal(ctx.mx_gemm_inner(dx, dy), ref)
        assert np.array_equal(ctx.mx_gemm_inner(dy, dx), ref.T)
    finally:
        ctx.set_exact_max(EXACT_MAX_DEFAULT)


def test_f64_pairs_forward_to_the_f64_entry_points(ctx, pool):
    n = 100_003
    r = np.random.default_rng(3)
    x, y = [r.uniform(-1, 1, n) for _ in range(3)], [r.uniform(-1, 1, n) for _ in range(2)]
    dx, dy = [pool.up(v) for v in x], [pool.up(v) for v in y]
    assert np.array_equal(ctx.mx_gemm_inner(dx, dy), ctx.gemm_inner(dx, dy))
    assert ctx.mx_dot(dx[0], dy[0]) == ctx.dot(dx[0], dy[0])
    al = r.uniform(-1, 1, (3, 2))
    a, b = [pool.up(v) for v in y], [pool.up(v) for v in y]
    ctx.mx_gemm_outer(al, dx, a)
    ctx.gemm_outer(al, dx, b)
    assert all(np.array_equal(u.numpy(), v.numpy()) for u, v in zip(a, b))


def test_ledger_counts_storage_bytes(ctx, pool):
    ctx.set_exact_max(0)
    try:
        n = 100_000
        x = [pool.up(np.ones(n), F32) for _ in range(6)]
        y = [pool.up(np.ones(n)) for _ in range(2)]
        ctx.ledger_reset()
        ctx.ledger_enable(True)
        ctx.mx_gemm_outer(np.ones((6, 2)), x, y)
        ctx.mx_gemm_outer(np.ones((6, 2)), x, y, set=True)
        ctx.mx_gemm_inner(y, x)
        ctx.mx_dot(x[0], y[0])
        ctx.mx_axpy(1.0, x[0], y[0])
        ctx.mx_copy(x[0], y[0])
        ctx.fill(1.0, x[0])
        ctx.scal(2.0, x[0])
        ctx.synchronize()
        led = ctx.ledger()
        ctx.ledger_enable(False)
        assert led["gemm_outer_f32"]["bytes"] == n * (4 * 6 + 16 * 2) + n * (4 * 6 + 8 * 2)
        assert led["gemm_inner_f32"]["bytes"] == n * (4 * 6 + 8 * 2)
        assert led["dot_f32"]["bytes"] == 12 * n
        assert led["axpy_f32"]["bytes"] == 20 * n
        assert led["copy_f32"]["bytes"] == 12 * n
        assert led["fill_f32"]["bytes"] == 4 * n
        assert led["scal_f32"]["bytes"] == 8 * n
    finally:
        ctx.ledger_enable(False)
        ctx.set_exact_max(EXACT_MAX_DEFAULT)


# ---- 6. solver: Davidson with the Q space stored in f32 -------------------------------------------
@pytest.fixture(scope="module")
def dense_3000():
    """H = (B + B^T) / 2 with B uniform(-0.01, 0.01), diagonal 1 + 9 i / n; and |H|_2."""
    n = 3000
    b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
    return h, float(np.max(np.abs(np.linalg.eigvalsh(h))))


def test_davidson_with_f32_q_space_matches_the_f64_run(ctx, dense_3000):
    """Storage rounding perturbs each stored vector by a relative eps32 / 2, so to first order an
    eigenvalue moves by at most 4 eps32 |H|_2 (Q parameters and Q actions, both signs), and the true
    residual of a converged root sits within the same distance of the threshold."""
    import itsolv_hbm as ih

    h, norm2 = dense_3000
    kw = dict(nroots=3, convergence_threshold=1e-6)
    f64 = ih.davidson_dense(ctx, h, **kw)
    q32 = ih.davidson_dense(ctx, h, q32=True, **kw)
    bound = 4 * EPS32 * norm2
    diff = np.max(np.abs(q32["eigenvalues"] - f64["eigenvalues"]))
    print(f"\nq32 davidson n=3000: iterations f64 {f64['iterations']} q32 {q32['iterations']}, "
          f"max |theta_q32 - theta_f64| {diff:.3e} (bound {bound:.3e}), q32 residual norms {q32['residual_norms']}, "
          f"f64 residual norms {f64['residual_norms']}")
    assert f64["converged"] and q32["converged"]
    assert diff <= bound
    assert np.all(q32["residual_norms"] <= 1e-6 + bound)
    assert q32["iterations"] <= f64["iterations"] + 3


def test_davidson_with_f32_q_space_on_the_exact_path(ctx):
    """Fixture bh (n = 28: every vector on the short-vector path) with 2 roots."""
    import itsolv_hbm as ih
    from test_solver_gpu import hamiltonian

    h = hamiltonian("bh", 1e-8)
    kw = dict(nroots=2, convergence_threshold=1e-6)
    f64 = ih.davidson_dense(ctx, h, **kw)
    q32 = ih.davidson_dense(ctx, h, q32=True, **kw)
    bound = 4 * EPS32 * float(np.max(np.abs(np.linalg.eigvalsh((h + h.T) / 2))))
    diff = np.max(np.abs(q32["eigenvalues"] - f64["eigenvalues"]))
    print(f"\nq32 davidson bh: iterations f64 {f64['iterations']} q32 {q32['iterations']}, max diff {diff:.3e} "
          f"(bound {bound:.3e})")
    assert f64["converged"] and q32["converged"]
    assert diff <= bound


def test_davidson_synthetic_with_f32_q_space(ctx):
    """The sharded-capable synthetic entry point on the bandwidth kernels (n = 100003, 4 roots)."""
    import itsolv_hbm as ih

    n, rho, rank, seed = 100_003, 0.1, 2, 20251015
    kw = dict(nroots=4, convergence_threshold=1e-6, max_size_qspace=24, reset_D=8)
    f64 = ih.davidson_synthetic(ctx, n, rho, rank, seed, **kw)
    q32 = ih.davidson_synthetic(ctx, n, rho, rank, seed, q32=True, **kw)
    norm2 = 1.0 + n + rank * rho * n  # |diag(1 + g)| + rho sum_l |u_l|^2
    assert f64["converged"] and q32["converged"]
    assert q32["iterations"] > 1 and q32["q_creations"] > 0  # the f32 Q space was built and read
    assert np.max(np.abs(q32["eigenvalues"] - f64["eigenvalues"])) <= 4 * EPS32 * norm2
    assert q32["iterations"] <= f64["iterations"] + 3
