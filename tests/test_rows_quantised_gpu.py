"""ssp_rows_export_quantised (csrc/kernels_rows.hip): the export whose first mq rows are rounded through
binary32 as they are stored, dst[k] = (double)(float)(xs[k] * src[k]).  A product and one rounding to nearest
even have exactly one correct answer, so every comparison is bit for bit (view(np.uint64) equality) against
two references: numpy's (x * s).astype(float32).astype(float64), and the library's own ssp_quantise_f32 on
copies of the vectors followed by ssp_rows_export.  There is no tolerance anywhere in this file.

The geometries are those of tests/test_rows_gpu.py (any base, any ld >= n, rows at 0 or 8 mod 16, the whole
sentinel-filled allocation compared), the values those of tests/test_q32_refined_gpu.py's specials(): ties of
both parities, binary32 subnormals, +-FLT_MAX, overflow to inf, signed zeros -- planted as special / s for every
scale, so the products land on them.

Up to n = 4099 every (ld, base) x (scale set) x mq runs.  At n = 2^20 + 5 a download of the allocation
dominates, so the (scale set, mq) pairs are dealt over the 6 geometries instead (every pair once, every
geometry with at least one): a row's path depends on its own (parity, scale == 1, k < mq) only, never on
the pair as a whole."""
import ctypes as C

import numpy as np
import pytest

from test_q32_refined_gpu import specials
from test_rows_gpu import LENGTHS, ROWS, SCALES, SENTINEL, Block, same, scale_sets

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered")]
F32, F64 = np.float32, np.float64

assert LENGTHS == [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 2**20 + 5]
assert ROWS == [1, 2, 3, 16, 17] and SCALES == [1.0, 0.3, -2.0**-30]


def quantised(p):
    with np.errstate(over="ignore"):
        return p.astype(F32).astype(F64)


def values(m, n, seed):
    """Uniform values over seven decades with the specials planted as special / s for each scale (for a scale
    that is no power of two the product lands within an f64 ulp of the special)."""
    r = np.random.default_rng(seed)
    x = r.uniform(-2, 2, (m, n)) * 10.0 ** r.integers(-3, 4, (m, n))
    sp = specials()
    with np.errstate(over="ignore"):
        plant = np.concatenate([sp / s for s in SCALES])
    for k in range(m):
        cnt = min(n, plant.size)
        x[k, r.permutation(n)[:cnt]] = np.roll(plant, 5 * k)[:cnt]
    return x


def mq_values(m):
    return sorted({0, 1, m - 1, m})


@pytest.fixture(params=[None, 0], ids=["exact_default", "exact_off"])
def xctx(ctx, request):
    if request.param is not None:
        ctx.set_exact_max(request.param)
    yield ctx
    ctx.set_exact_max(2048)


def check_export(ctx, vecs, tmp, x, products, rounded, dst, ref, xs, mq, where):
    m = len(vecs)
    s = [1.0] * m if xs is None else xs
    ctx.fill(SENTINEL, dst.buf)
    ctx.rows_export_quantised(vecs, dst.rows, xs, mq)
    got = dst.buf.numpy()
    want = [(rounded if k < mq else products)[s[k]][k] for k in range(m)]
    assert same(got, dst.expect(want)), ("numpy", where)
    # the library's own two passes: quantise copies of the first mq vectors, then the plain export
    for k in range(mq):
        ctx.copy(tmp[k], vecs[k])
    if mq:
        ctx.quantise_f32(tmp[:mq], s[:mq])
    ctx.fill(SENTINEL, ref.buf)
    ctx.rows_export(tmp[:mq] + vecs[mq:], ref.rows, [1.0] * mq + s[mq:])
    assert same(got, ref.buf.numpy()), ("quantise_f32 + rows_export", where)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", LENGTHS)
def test_export_quantised_matches_numpy_and_the_two_pass_route(xctx, n, m):
    ctx = xctx
    x = values(m, n, 100 * m + n % 97)
    with np.errstate(over="ignore"):
        products = {s: (x if s == 1.0 else x * s) for s in SCALES}
    rounded = {s: quantised(p) for s, p in products.items()}
    if n >= 69:  # every special fits: the planted classes are really among the rounded products
        w = np.concatenate([rounded[s][0] for s in SCALES])
        assert np.any(np.isinf(w)) and np.any(np.signbit(w) & (w == 0))
        assert np.any((np.abs(w) > 0) & (np.abs(w) < np.finfo(F32).tiny)) and np.any(np.abs(w) == np.finfo(F32).max)
    vecs = [ctx.upload(x[k]) for k in range(m)]
    tmp = [ctx.alloc(n) for _ in range(m)]
    geometries = [(ld, base) for ld in (n, n + 1, n + 3) for base in (0, 1)]
    pairs = [(xs, mq) for xs in scale_sets(m) + [None] for mq in mq_values(m)]
    for g, (ld, base) in enumerate(geometries):
        dst, ref = Block(ctx, m, n, ld, base), Block(ctx, m, n, ld, base)
        for xs, mq in (pairs if n <= 4099 else pairs[g::len(geometries)]):
            check_export(ctx, vecs, tmp, x, products, rounded, dst, ref, xs, mq, (n, m, ld, base, xs, mq))
        dst.free()
        ref.free()
    for k in range(m):
        assert same(vecs[k].numpy(), x[k]), ("a source was written", n, m, k)
    for v in vecs + tmp:
        v.free()


@pytest.mark.parametrize("n", [2**24 - 3, 2**24 + 3])
def test_both_parities_on_each_side_of_the_window_threshold(ctx, n):
    """m = 2 with an odd ld: row 0 aligned, row 1 at 8 mod 16; each rounded and not, with and without a scale."""
    m, ld = 2, n + 1
    r = np.random.default_rng(n % 1000)
    x = r.uniform(-2, 2, (m, n))
    sp = specials()
    for k in range(m):
        x[k, :sp.size] = np.roll(sp, k)
        x[k, -sp.size:] = np.roll(sp, k + 1) / 0.3
        x[k, n // 2 + k:n // 2 + k + sp.size] = sp / -2.0**-30
    vecs = [ctx.upload(x[k]) for k in range(m)]
    dst = Block(ctx, m, n, ld, 0)
    for xs, mq in (([1.0, 0.3], 2), ([-2.0**-30, 1.0], 2), ([0.3, 0.3], 1), ([1.0, 1.0], 0)):
        ctx.rows_export_quantised(vecs, dst.rows, xs, mq)
        with np.errstate(over="ignore"):
            want = [x[k] if xs[k] == 1.0 else x[k] * xs[k] for k in range(m)]
        want = [quantised(w) if k < mq else w for k, w in enumerate(want)]
        assert same(dst.buf.numpy(), dst.expect(want)), (xs, mq)
    for k in range(m):
        assert same(vecs[k].numpy(), x[k]), k
    dst.free()
    for v in vecs:
        v.free()


@pytest.mark.parametrize("m", ROWS)
def test_ledger_counts_one_entry_per_launch(ctx, m):
    n = 257
    blk = Block(ctx, m, n, n + 1, 1)
    vecs = [ctx.upload(r) for r in values(m, n, m)]
    ctx.ledger_enable(True)
    try:
        ctx.ledger_reset()
        ctx.rows_export_quantised(vecs, blk.rows, [0.3] * m, max(0, m - 1))
        ctx.synchronize()
        led = ctx.ledger()
    finally:
        ctx.ledger_enable(False)
    assert set(led) == {"rows_export_q"}, led
    assert led["rows_export_q"]["calls"] == (1 if m <= 16 else 2), led
    assert led["rows_export_q"]["bytes"] == 16.0 * m * n, led
    for v in vecs:
        v.free()
    blk.free()


def test_arguments(ctx):
    import subspace_hip as sh

    n = 8
    lib, h = ctx.lib, ctx.handle
    buf = ctx.upload(np.arange(3.0 * n + 2))
    v = ctx.upload(np.full(n, -1.0))
    two = (C.c_void_p * 2)(v.ptr, v.ptr)
    for mq in (-1, 3):
        assert lib.ssp_rows_export_quantised(h, two, None, 2, mq, buf.ptr, n, n) == 3, mq
        assert b"mq" in lib.ssp_last_error()
    assert lib.ssp_rows_export_quantised(h, two, None, -1, 0, buf.ptr, n, n) == 3
    assert lib.ssp_rows_export_quantised(h, two, None, 2, 1, buf.ptr, n - 1, n) == 3  # ld < n
    assert lib.ssp_rows_export_quantised(h, two, None, 2, 1, None, n, n) == 3
    assert lib.ssp_rows_export_quantised(h, None, None, 0, 0, None, 0, n) == 0  # nothing to do
    assert lib.ssp_rows_export_quantised(h, two, None, 2, 2, buf.ptr, 0, 0) == 0
    assert same(buf.numpy(), np.arange(3.0 * n + 2)) and same(v.numpy(), np.full(n, -1.0))
    with pytest.raises(ValueError):
        ctx.rows_export_quantised([v] * 4, sh.DeviceRows(ctx, 2, n, ptr=buf.ptr))
    assert {"ssp_rows_export_quantised"} == set(sh.OPTIONAL_ROWS_Q) <= set(sh.EXPORTS)
    buf.free()
    v.free()
