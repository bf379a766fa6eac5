"""ssp_rows_import / ssp_rows_export (csrc/kernels_rows.hip): a caller's row-major device block into and out
of library vectors.  A copy and a single product have exactly one correct answer, so every comparison is
bit for bit against numpy (view(np.uint64) equality); there is no tolerance anywhere in this file.

The caller's block is any double* base and any ld >= n, so its rows sit at 0 or 8 mod 16; an odd ld
alternates.  Every geometry below is laid out inside a larger allocation filled with a sentinel, and the
whole allocation is compared afterwards: the padding [n, ld) of every row, the elements before the base
and the elements after the last row must come back untouched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 2**20 + 5]
ROWS = [1, 2, 3, 16, 17]  # 17 crosses a launch
SCALES = [1.0, 0.3, -2.0**-30]
SENTINEL = -7.25e300
TAIL = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def specials():
    """Signed zeros, subnormals (the smallest, the largest, one whose product with 0.3 and 2^-30 rounds inside
    the subnormal range or to zero), the extremes of the normal range and both infinities."""
    tiny = np.finfo(np.float64).tiny
    return np.array([0.0, -0.0, 5e-324, -5e-324, tiny * (1 - 2.0**-52), tiny / 3, -tiny / 7, tiny, 2.0**-1040,
                     np.finfo(np.float64).max, -np.finfo(np.float64).max, np.inf, -np.inf, 1.0, -1.0])


def values(m, n, seed):
    r = np.random.default_rng(seed)
    x = r.uniform(-2, 2, (m, n)) * 10.0 ** r.integers(-3, 4, (m, n))
    sp = specials()
    for k in range(m):
        cnt = min(n, sp.size)
        x[k, r.permutation(n)[:cnt]] = np.roll(sp, k)[:cnt]
    return x


class Block:
    """A caller's block inside an allocation of sentinels: row k at element base + k * ld."""

    def __init__(self, ctx, m, n, ld, base, rows=None):
        import subspace_hip as sh

        self.m, self.n, self.ld, self.base = m, n, ld, base
        self.image = np.full(base + (m - 1) * ld + n + TAIL, SENTINEL)
        if rows is not None:
            self.set_rows(self.image, rows)
        self.buf = ctx.upload(self.image)
        self.rows = sh.DeviceRows(ctx, m, n, ld, ptr=self.buf.ptr + 8 * base)

    def set_rows(self, image, rows):
        for k in range(self.m):
            image[self.base + k * self.ld:self.base + k * self.ld + self.n] = rows[k]

    def expect(self, rows):
        e = np.full(self.image.size, SENTINEL)
        self.set_rows(e, rows)
        return e

    def free(self):
        self.buf.free()


@pytest.fixture(params=[None, 0], ids=["exact_default", "exact_off"])
def xctx(ctx, request):
    """The session context with exact_max at its default and at 0 (copies look at neither)."""
    if request.param is not None:
        ctx.set_exact_max(request.param)
    yield ctx
    ctx.set_exact_max(2048)


def scale_sets(m):
    mixed = [SCALES[(k + 1) % 3] for k in range(m)]
    return [[s] * m for s in SCALES] + [mixed]


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n", LENGTHS)
def test_import_and_export_are_bit_copies_and_single_products(xctx, n, m):
    ctx = xctx
    x = values(m, n, 100 * m + n % 97)
    vecs = [ctx.alloc(n) for _ in range(m)]
    w = ctx.alloc(n)
    sets = scale_sets(m) + [None]  # None: no scale array at all
    products = {s: x * s for s in SCALES[1:]}
    for ld in (n, n + 1, n + 3):
        for base in (0, 1):
            src = Block(ctx, m, n, ld, base, x)
            for v in vecs:
                ctx.fill(SENTINEL, v)
            ctx.rows_import(src.rows, vecs)
            for k in range(m):
                assert same(vecs[k].numpy(), x[k]), ("import", n, m, ld, base, k)
            assert same(src.buf.numpy(), src.image), ("import changed its source", n, m, ld, base)
            src.free()
            dst = Block(ctx, m, n, ld, base)
            for xs in sets:
                ctx.fill(SENTINEL, dst.buf)
                ctx.rows_export(vecs, dst.rows, xs)
                got = dst.buf.numpy()
                s = [1.0] * m if xs is None else xs
                want = [x[k] if s[k] == 1.0 else products[s[k]][k] for k in range(m)]
                assert same(got, dst.expect(want)), ("export", n, m, ld, base, xs)
                # ... and the library's scaled copy into an aligned vector, read back (the long vectors:
                # the first and the last row)
                for k in (range(m) if n <= 4099 else sorted({0, m - 1})):
                    ctx.scal_copy(s[k], w, vecs[k])
                    row = got[base + k * ld:base + k * ld + n]
                    assert same(row, w.numpy()), ("scal_copy", n, m, ld, base, k)
            dst.free()
    for v in vecs + [w]:
        v.free()


@pytest.mark.parametrize("n", [2**24 - 3, 2**24 + 3])
def test_both_parities_on_each_side_of_the_window_threshold(ctx, n):
    """k_copy's rule: the window shape with nontemporal accesses from 2^24 elements.  m = 2 with an odd ld:
    row 0 aligned, row 1 at 8 mod 16; each with and without a scale."""
    m, ld = 2, n + 1
    r = np.random.default_rng(n % 1000)
    x = r.uniform(-2, 2, (m, n))
    sp = specials()
    for k in range(m):
        x[k, :sp.size] = np.roll(sp, k)
        x[k, -sp.size:] = np.roll(sp, k + 1)
        x[k, n // 2 + k:n // 2 + k + sp.size] = sp
    vecs = [ctx.alloc(n) for _ in range(m)]
    src = Block(ctx, m, n, ld, 0, x)
    ctx.rows_import(src.rows, vecs)
    for k in range(m):
        assert same(vecs[k].numpy(), x[k]), ("import", k)
    src.free()
    for xs in ([1.0, 0.3], [-2.0**-30, 1.0]):
        dst = Block(ctx, m, n, ld, 0)
        ctx.rows_export(vecs, dst.rows, xs)
        want = [x[k] if xs[k] == 1.0 else x[k] * xs[k] for k in range(m)]
        assert same(dst.buf.numpy(), dst.expect(want)), xs
        dst.free()
    for v in vecs:
        v.free()


@pytest.mark.parametrize("m", ROWS)
def test_ledger_counts_one_launch_for_sixteen_rows(ctx, m):
    n = 257
    x = values(m, n, m)
    blk = Block(ctx, m, n, n + 1, 1, x)
    vecs = [ctx.alloc(n) for _ in range(m)]
    ctx.ledger_enable(True)
    try:
        ctx.ledger_reset()
        ctx.rows_import(blk.rows, vecs)
        ctx.rows_export(vecs, blk.rows, [0.3] * m)
        ctx.synchronize()
        led = ctx.ledger()
    finally:
        ctx.ledger_enable(False)
    launches = 1 if m <= 16 else 2
    for name in ("rows_import", "rows_export"):
        assert led[name]["calls"] == launches, (name, led[name])
        assert led[name]["bytes"] == 16.0 * m * n, (name, led[name])
    assert set(led) == {"rows_import", "rows_export"}, led
    for v in vecs:
        v.free()
    blk.free()


@pytest.mark.parametrize("n", [4099, 2**20 + 5])
def test_a_pending_zero_fill_is_honoured_on_both_sides(ctx, n):
    """The pattern of test_quantise_stores_a_pending_zero_fill_first: ssp_fill(+0.0) of a vector longer than
    exact_max is recorded, not launched (csrc/pending_fill.h)."""
    import subspace_hip as sh

    x = values(2, n, 5)
    rows = sh.DeviceRows(ctx, 2, n)  # aligned rows of one owned allocation
    v, w = ctx.upload(np.full(n, 3.5)), ctx.upload(x[1])
    # import: a destination's recorded fill is dropped, not stored after the copy
    rows.upload(x)
    ctx.fill(0.0, v)
    ctx.rows_import(rows, [v])
    ctx.synchronize()
    assert same(v.numpy(), x[0])
    # import: a source row's recorded fill is stored before the row is read
    ctx.fill(0.0, rows.row(0))
    ctx.rows_import(rows, [v, w])
    assert same(v.numpy(), np.zeros(n)) and same(w.numpy(), x[1])
    # export: a source's recorded fill is stored first (+0 * 0.5 = +0)
    rows.upload(x)
    ctx.upload_into(v, x[0])
    ctx.fill(0.0, v)
    ctx.rows_export([v, w], rows, [0.5, 1.0])
    got = rows.numpy()
    assert same(got[0], np.zeros(n)) and same(got[1], x[1])
    # export: a fill recorded for a destination row is dropped, not stored over the result
    ctx.upload_into(v, x[0])
    ctx.fill(0.0, rows.row(1))
    ctx.rows_export([v, w], rows)
    ctx.synchronize()
    assert same(rows.numpy(), x)
    rows.free()
    # export: a recorded fill that the rows only partly cover (the whole allocation, padding included) is
    # stored first, then the rows are written
    blk = Block(ctx, 2, n, n + 1, 1)
    ctx.fill(0.0, blk.buf)
    ctx.rows_export([v, w], blk.rows, [1.0, -2.0**-30])
    want = np.zeros(blk.image.size)
    blk.set_rows(want, [x[0], x[1] * -2.0**-30])
    assert same(blk.buf.numpy(), want)
    blk.free()
    v.free()
    w.free()


def test_argument_errors_name_their_cause(ctx):
    n = 8
    lib, h = ctx.lib, ctx.handle
    buf = ctx.upload(np.arange(3.0 * n + 2))
    v = ctx.upload(np.full(n, -1.0))
    one = (C.c_void_p * 1)(v.ptr)
    off = (C.c_void_p * 1)(v.ptr + 8)
    null = (C.c_void_p * 1)(None)

    def err(code, word):
        assert code == 3, code
        assert word.encode() in lib.ssp_last_error(), lib.ssp_last_error()

    err(lib.ssp_rows_import(h, buf.ptr, n, one, -1, n), "negative")
    err(lib.ssp_rows_export(h, one, None, -1, buf.ptr, n, n), "negative")
    err(lib.ssp_rows_import(h, buf.ptr, n - 1, one, 1, n), "ld")
    err(lib.ssp_rows_export(h, one, None, 1, buf.ptr, n - 1, n), "ld")
    err(lib.ssp_rows_import(h, None, n, one, 1, n), "null")
    err(lib.ssp_rows_export(h, one, None, 1, None, n, n), "null")
    err(lib.ssp_rows_import(h, buf.ptr, n, None, 1, n), "null")
    err(lib.ssp_rows_import(h, buf.ptr, n, null, 1, n), "null")
    err(lib.ssp_rows_export(h, null, None, 1, buf.ptr, n, n), "null")
    err(lib.ssp_rows_import(h, buf.ptr, n, off, 1, n - 1), "16-byte aligned")
    err(lib.ssp_rows_export(h, off, None, 1, buf.ptr, n, n - 1), "16-byte aligned")
    err(lib.ssp_rows_import(h, buf.ptr + 4, n, one, 1, n), "8-byte aligned")
    # nothing to do: SSP_OK, whatever else is passed, and nothing is written
    assert lib.ssp_rows_import(h, None, 0, None, 0, n) == 0
    assert lib.ssp_rows_import(h, buf.ptr, 0, one, 1, 0) == 0
    assert lib.ssp_rows_export(h, None, None, 0, None, 0, n) == 0
    assert lib.ssp_rows_export(h, one, None, 1, buf.ptr, 0, 0) == 0
    assert same(v.numpy(), np.full(n, -1.0)) and same(buf.numpy(), np.arange(3.0 * n + 2))
    buf.free()
    v.free()


def test_device_rows_owns_one_aligned_allocation(ctx):
    import subspace_hip as sh

    a = values(3, 7, 1)
    rows = sh.DeviceRows(ctx, 3, 7)
    assert rows.ld == 8 and len(rows) == 3 and all(rows.row(k).ptr % 16 == 0 and not rows.row(k).owner for k in range(3))
    rows.upload(a)
    assert same(rows.numpy(), a) and same(rows.row(1).numpy(), a[1])
    ctx.scal(2.0, rows.row(2))  # a row goes to any Context op
    assert same(rows.head(2).numpy(), a[:2]) and same(rows.row(2).numpy(), 2.0 * a[2])
    with pytest.raises(ValueError):
        sh.DeviceRows(ctx, 2, 8, 7)
    with pytest.raises(ValueError):
        ctx.rows_import(rows, [rows.row(0)] * 4)
    in_use = ctx.memory_stats()[0]
    rows.free()
    assert ctx.memory_stats()[0] < in_use and rows.ptr == 0
    assert {"ssp_rows_import", "ssp_rows_export"} == set(sh.OPTIONAL_ROWS) <= set(sh.EXPORTS)
