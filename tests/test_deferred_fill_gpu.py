"""Deferred zero fills (iterative-solver_amd/csrc/pending_fill.h): ssp_fill(+0.0) is recorded, not
launched, and the next ssp_gemm_outer whose destinations are exactly the recorded vectors starts its
accumulators from zero (the write-only SET kernel) instead of reading the zeros back.

Every result is compared bit for bit (np.array_equal) with the same calls on a second context created
with SSP_DEFER_FILL=0, which launches every fill at once.  The fused cases are also held to the oracle
at the bound tests/test_ops_gpu.py::test_gemm_outer uses.  Vectors hold random data before they are
filled, so a fill that was dropped instead of stored shows.

The ledger tells the paths apart: a stored fill is a "fill" row; a consumed one leaves none, and the
"gemm_outer" row then carries 8 n (k + m) bytes instead of the read-modify-write 8 n (k + 2 m).
(Reading the ledger is itself an entry point that stores pending fills, so "still pending" is shown
by what a following gemm_outer does.)

Shapes: n just above the exact-mode limit (2048), odd tails, whole and part wave windows of 512
doubles; m across kOuterDst = 16; k across the 4-source groups, their remainder and kOuterSrc = 64.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NS = [2049, 2560, 4099, 70001]
MS = [1, 3, 8, 17]
KS = [1, 4, 5, 48, 65]
KMAX, MMAX = max(KS), max(MS)


class Side:
    """One context with the sources of every n uploaded once."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.src = {}

    def sources(self, n):
        if n not in self.src:
            self.src[n] = [self.ctx.upload(v) for v in host_sources(n)]
        return self.src[n]


_host = {}


def host_sources(n):
    if n not in _host:
        r = np.random.default_rng(n)
        _host[n] = [r.uniform(-1, 1, n) for _ in range(KMAX)]
    return _host[n]


def coef(k, m):
    return np.random.default_rng(1000 * k + m).uniform(-1, 1, (k, m))


@pytest.fixture(scope="module")
def sides():
    import subspace_hip as sh

    if sh.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X")
    old = os.environ.pop("SSP_DEFER_FILL", None)
    try:
        deferred = sh.Context(0)
        os.environ["SSP_DEFER_FILL"] = "0"
        eager = sh.Context(0)
    finally:
        os.environ.pop("SSP_DEFER_FILL", None)
        if old is not None:
            os.environ["SSP_DEFER_FILL"] = old
    for c in (deferred, eager):
        c.ledger_enable(True)
    yield Side(deferred), Side(eager)
    deferred.close()
    eager.close()


def garbage(ctx, n, seed=0):
    """A vector that holds data, so that a missing store of zeros shows."""
    return ctx.upload(np.random.default_rng(77 + seed).uniform(1, 2, n))


def view(ctx, v, off, n):
    import subspace_hip as sh

    return sh.DeviceVector(ctx, n, v.ptr + 8 * off, owner=False)


def both(sides, fn):
    """fn(side) -> (arrays, ledger) on the deferring and on the eager context; the arrays must agree
    bit for bit.  Returns the deferring side's arrays and both ledgers."""
    out = []
    for s in sides:
        s.ctx.ledger_reset()
        arrays = fn(s)
        out.append(([np.asarray(a) for a in arrays], s.ctx.ledger()))
    (da, dl), (ea, el) = out
    assert len(da) == len(ea)
    for a, b in zip(da, ea):
        assert a.shape == b.shape and np.array_equal(a, b)
        assert np.array_equal(np.signbit(a), np.signbit(b))  # array_equal takes -0.0 for +0.0
    return da, dl, el


def calls(ledger, op):
    return ledger.get(op, {"calls": 0})["calls"]


def outer_bound(al, xs, y0=None):
    """tests/test_ops_gpu.py::test_gemm_outer: |got - oracle| <= 4 k eps (|y| + sum_i |alpha_i| |x_i|)."""
    k = al.shape[0]
    terms = np.abs(al).T @ np.abs(np.array(xs))
    if y0 is not None:
        terms = terms + np.abs(np.array(y0))
    return 4 * k * EPS * terms


# 1. fill(0) x m then gemm_outer: consumed
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_fill_then_gemm_outer_is_one_write_only_pass(sides, n, m, k):
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        dst = [garbage(c, n, j) for j in range(m)]
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src[:k], dst)
        got = [v.numpy() for v in dst]
        for v in dst:
            v.free()
        return got

    got, dl, el = both(sides, run)
    assert calls(dl, "fill") == 0 and calls(el, "fill") == m
    assert calls(dl, "gemm_outer") == 1 and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + m)
    assert calls(el, "gemm_outer") == 1 and el["gemm_outer"]["bytes"] == 8.0 * n * (k + 2 * m)
    assert "gemm_outer_set" not in dl  # the row keeps the name of the call made
    xs = host_sources(n)[:k]
    ref = oracle.gemm_outer(al, xs, [np.zeros(n) for _ in range(m)])
    bound = outer_bound(al, xs)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


def test_exact_mode_vectors_are_not_deferred(sides):
    n, m, k = 2048, 3, 5  # n <= exact_max: the reference's arithmetic, fills launched at once
    al = coef(k, m)

    def run(s):
        c = s.ctx
        xs = [c.upload(v[:n]) for v in host_sources(NS[0])[:k]]
        dst = [garbage(c, n, j) for j in range(m)]
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, xs, dst)
        got = [v.numpy() for v in dst]
        for v in dst + xs:
            v.free()
        return got

    got, dl, el = both(sides, run)
    for led in (dl, el):
        assert calls(led, "fill") == m and led["gemm_outer"]["bytes"] == 8.0 * n * (k + 2 * m)
    xs = [v[:n] for v in host_sources(NS[0])[:k]]
    ref = oracle.gemm_outer(al, xs, [np.zeros(n) for _ in range(m)])
    bound = outer_bound(al, xs)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 2. some destinations filled, others holding data: all or nothing
@pytest.mark.parametrize("n,m,k", [(2049, 3, 5), (4099, 8, 48), (70001, 17, 65)])
def test_partly_filled_destinations_fall_back_to_read_modify_write(sides, n, m, k):
    al = coef(k, m)
    filled = [j for j in range(m) if j % 2 == 0]
    y0 = [np.random.default_rng(500 + j).uniform(-1, 1, n) for j in range(m)]

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        dst = [c.upload(v) for v in y0]
        c.ledger_reset()
        for j in filled:
            c.fill(0.0, dst[j])
        c.gemm_outer(al, src[:k], dst)
        got = [v.numpy() for v in dst]
        for v in dst:
            v.free()
        return got

    got, dl, el = both(sides, run)
    assert calls(dl, "fill") == len(filled) and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + 2 * m)
    start = [np.zeros(n) if j in filled else y0[j] for j in range(m)]
    xs = host_sources(n)[:k]
    ref = oracle.gemm_outer(al, xs, start)
    bound = outer_bound(al, xs, start)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 3. a destination view inside a filled range
@pytest.mark.parametrize("n,off,nv", [(4099, 512, 2049), (70001, 1026, 4099)])
def test_destination_view_inside_a_filled_range(sides, n, off, nv):
    k = 5
    al = coef(k, 1)

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        big = garbage(c, n)
        xs = [view(c, v, 0, nv) for v in src[:k]]
        c.ledger_reset()
        c.fill(0.0, big)
        c.gemm_outer(al, xs, [view(c, big, off, nv)])
        got = big.numpy()
        big.free()
        return [got]

    (got,), dl, el = both(sides, run)
    assert calls(dl, "fill") == 1 and dl["gemm_outer"]["bytes"] == 8.0 * nv * (k + 2)
    xs = [v[:nv] for v in host_sources(n)[:k]]
    ref = oracle.gemm_outer(al, xs, [np.zeros(nv)])[0]
    assert np.all(np.abs(got[off:off + nv] - ref) <= outer_bound(al, xs)[0])
    assert not got[:off].any() and not got[off + nv:].any()


# 4. a filled vector used as a source
@pytest.mark.parametrize("dst_filled", [False, True])
def test_filled_vector_as_a_source(sides, dst_filled):
    n, m, k = 4099, 3, 5
    al = coef(k, m)
    y0 = [np.random.default_rng(600 + j).uniform(-1, 1, n) for j in range(m)]

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        z = garbage(c, n)
        dst = [c.upload(v) for v in y0]
        xs = src[:k - 1]
        xs = xs[:2] + [z] + xs[2:]
        c.ledger_reset()
        c.fill(0.0, z)
        if dst_filled:
            for v in dst:
                c.fill(0.0, v)
        c.gemm_outer(al, xs, dst)
        got = [v.numpy() for v in dst] + [z.numpy()]
        for v in dst + [z]:
            v.free()
        return got

    got, dl, el = both(sides, run)
    # the source's fill is stored; the destinations' fills are still consumed
    assert calls(dl, "fill") == 1
    assert dl["gemm_outer"]["bytes"] == 8.0 * n * (k + (1 if dst_filled else 2) * m)
    assert not got[m].any()
    h = host_sources(n)[:k - 1]
    xs = h[:2] + [np.zeros(n)] + h[2:]
    start = [np.zeros(n) for _ in range(m)] if dst_filled else y0
    ref = oracle.gemm_outer(al, xs, start)
    bound = outer_bound(al, xs, start)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 5. the same destination twice
def test_same_destination_twice_is_not_consumed(sides):
    n, k = 2560, 4
    al = coef(k, 2)

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        y = garbage(c, n)
        c.ledger_reset()
        c.fill(0.0, y)
        c.gemm_outer(al, src[:k], [y, y])
        got = y.numpy()
        y.free()
        return [got]

    _, dl, el = both(sides, run)
    assert calls(dl, "fill") == 1 and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + 4)


# 6. fill(0) followed by each reader that must see the zeros
def _allreduce(c, v):
    assert c.lib.ssp_allreduce_sum(c.handle, ctypes.c_void_p(v.ptr), v.n) == 0
    return v.numpy()


READERS = {
    "download": lambda c, z, x, y: [z.numpy()],
    "dot": lambda c, z, x, y: [c.dot(z, x), c.dot(z, z), z.numpy()],
    "gemm_inner_row": lambda c, z, x, y: [c.gemm_inner([z], [x, y]), z.numpy()],
    "gemm_inner_column": lambda c, z, x, y: [c.gemm_inner([x, y], [z]), z.numpy()],
    "axpy_as_x": lambda c, z, x, y: [c.axpy(0.5, z, y), y.numpy(), z.numpy()][1:],
    "axpy_as_y": lambda c, z, x, y: [c.axpy(-0.5, x, z), z.numpy()][1:],
    "scal": lambda c, z, x, y: [c.scal(-2.0, z), z.numpy()][1:],
    "copy_as_source": lambda c, z, x, y: [c.copy(y, z), y.numpy(), z.numpy()][1:],
    "select": lambda c, z, x, y: list(c.select(z, 5)) + [z.numpy()],
    "precondition": lambda c, z, x, y: [c.precondition([z], y, [0.25]), z.numpy()][1:],
    "allreduce_sum": lambda c, z, x, y: [_allreduce(c, z)],
}


@pytest.mark.parametrize("n", [2049, 70001])
@pytest.mark.parametrize("reader", sorted(READERS))
def test_fill_then_reader_sees_zeros(sides, reader, n):
    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        z, y = garbage(c, n, 1), garbage(c, n, 2)  # y in [1, 2): a safe preconditioner diagonal
        x = src[0]
        c.ledger_reset()
        c.fill(0.0, z)
        got = READERS[reader](c, z, x, y)
        for v in (z, y):
            v.free()
        return got

    got, dl, el = both(sides, run)
    assert calls(dl, "fill") == 1 and calls(el, "fill") == 1
    if reader == "axpy_as_y":
        assert np.array_equal(got[-1], -0.5 * host_sources(n)[0])
    elif reader not in ("axpy_as_x", "copy_as_source"):
        assert not np.asarray(got[-1]).any()  # z itself: zeros (scal, precondition and the sum keep them)
    if reader in ("axpy_as_x",):
        assert np.array_equal(got[0], np.random.default_rng(79).uniform(1, 2, n))  # y + 0.5 * 0
    if reader == "copy_as_source":
        assert not got[0].any() and not got[1].any()


# 7. fill(0) then fill(3.0): the zero fill is covered, never stored
def test_zero_fill_covered_by_a_later_fill(sides):
    n = 4099

    def run(s):
        c = s.ctx
        v = garbage(c, n)
        c.ledger_reset()
        c.fill(0.0, v)
        c.fill(3.0, v)
        got = v.numpy()
        v.free()
        return [got]

    (got,), dl, el = both(sides, run)
    assert np.array_equal(got, np.full(n, 3.0))
    assert calls(dl, "fill") == 1 and calls(el, "fill") == 2


# 8. fill(2.0) then gemm_outer: a non-zero fill is launched at once
def test_nonzero_fill_is_not_deferred(sides):
    n, m, k = 2560, 3, 4
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        dst = [garbage(c, n, j) for j in range(m)]
        c.ledger_reset()
        for v in dst:
            c.fill(2.0, v)
        c.gemm_outer(al, src[:k], dst)
        got = [v.numpy() for v in dst]
        for v in dst:
            v.free()
        return got

    got, dl, el = both(sides, run)
    assert calls(dl, "fill") == m and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + 2 * m)
    xs = host_sources(n)[:k]
    start = [np.full(n, 2.0) for _ in range(m)]
    ref = oracle.gemm_outer(al, xs, start)
    bound = outer_bound(al, xs, start)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 9. fill(-0.0) keeps its sign
def test_negative_zero_fill_keeps_the_sign_bit(sides):
    n, k = 2049, 1

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        v, w = garbage(c, n, 1), garbage(c, n, 2)
        c.ledger_reset()
        c.fill(-0.0, v)
        c.fill(-0.0, w)
        # not consumed: fma(0, x, -0.0) is -0.0 wherever 0 * x is, and a start from +0.0 never is
        c.gemm_outer(np.zeros((k, 1)), [src[0]], [w])
        got = [v.numpy(), w.numpy()]
        for u in (v, w):
            u.free()
        return got

    got, dl, el = both(sides, run)
    assert not got[0].any() and np.all(np.signbit(got[0]))
    assert calls(dl, "fill") == 2 and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + 2)


# 10. fill(0), free, alloc of the same size, upload, download
def test_freed_block_is_never_written_by_a_stale_fill(sides):
    n = 5003  # a block size no other test of this module frees, so the arena hands this block back
    data = np.random.default_rng(10).uniform(-1, 1, n)

    def run(s):
        c = s.ctx
        v = garbage(c, n)
        p = v.ptr
        c.ledger_reset()
        c.fill(0.0, v)
        v.free()
        w = c.alloc(n)
        assert w.ptr == p  # the arena recycles the block
        c.upload_into(w, data)
        c.synchronize()
        got = w.numpy()
        w.free()
        return [got]

    (got,), dl, el = both(sides, run)
    assert np.array_equal(got, data)
    assert calls(dl, "fill") == 0 and calls(el, "fill") == 1  # dropped with the block, never stored


# 11. more pending fills than the table holds
def test_hundred_pending_fills_are_all_stored(sides):
    n, count = 2049, 100

    def run(s):
        c = s.ctx
        vs = [garbage(c, n, i) for i in range(count)]
        c.ledger_reset()
        for v in vs:
            c.fill(0.0, v)
        got = [v.numpy() for v in vs]
        for v in vs:
            v.free()
        return got

    got, dl, el = both(sides, run)
    assert all(not g.any() for g in got)
    assert calls(dl, "fill") == count and calls(el, "fill") == count


# 12. taking the stream stores pending fills
def test_taking_the_stream_stores_pending_fills(sides):
    n, m, k = 2560, 3, 4
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        dst = [garbage(c, n, j) for j in range(m)]
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        assert c.stream  # the hand-off to foreign code: the zeros must be in memory behind it
        c.gemm_outer(al, src[:k], dst)  # would have consumed fills that were still pending
        got = [v.numpy() for v in dst]
        for v in dst:
            v.free()
        return got

    _, dl, el = both(sides, run)
    assert calls(dl, "fill") == m and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + 2 * m)


# 13. write-only ops onto a pending destination drop the fill
@pytest.mark.parametrize("n", [2049, 70001])
def test_write_only_ops_drop_the_pending_fill(sides, n):
    m, k = 3, 5
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        dst = [garbage(c, n, j) for j in range(m)]
        t, u = garbage(c, n, 8), garbage(c, n, 9)
        c.ledger_reset()
        for v in dst + [t, u]:
            c.fill(0.0, v)
        c.gemm_outer_set(al, src[:k], dst)
        c.copy(t, src[1])
        c.scal_copy(-3.0, u, src[2])
        got = [v.numpy() for v in dst + [t, u]]
        for v in dst + [t, u]:
            v.free()
        return got

    got, dl, el = both(sides, run)
    assert calls(dl, "fill") == 0 and calls(el, "fill") == m + 2
    xs = host_sources(n)
    ref = oracle.gemm_outer(al, xs[:k], [np.zeros(n) for _ in range(m)])
    bound = outer_bound(al, xs[:k])
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])
    assert np.array_equal(got[m], xs[1]) and np.array_equal(got[m + 1], -3.0 * xs[2])


def test_untouched_pending_fills_stay_pending(sides):
    n, k = 4099, 5
    al = coef(k, 1)

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        a, b = garbage(c, n, 1), garbage(c, n, 2)
        c.ledger_reset()
        c.fill(0.0, a)
        c.fill(0.0, b)
        c.gemm_outer(al, src[:k], [a])  # consumes a; b is no operand
        c.gemm_outer(al, src[:k], [b])  # b was still pending: consumed too
        got = [a.numpy(), b.numpy()]
        for v in (a, b):
            v.free()
        return got

    got, dl, el = both(sides, run)
    assert np.array_equal(got[0], got[1])
    assert calls(dl, "fill") == 0 and calls(dl, "gemm_outer") == 2
    assert dl["gemm_outer"]["bytes"] == 2 * 8.0 * n * (k + 1)



# deferred scales: source scales do not stand in the way, a destination scale does
@pytest.mark.parametrize("n,m,k", [(2049, 3, 5), (4099, 17, 65)])
@pytest.mark.parametrize("ys_kind", ["none", "ones", "scaled"])
def test_scaled_gemm_outer_consumes_only_without_destination_scales(sides, n, m, k, ys_kind):
    al = coef(k, m)
    xs_scale = np.random.default_rng(k).uniform(0.5, 2.0, k)
    ys_scale = {"none": None, "ones": np.ones(m), "scaled": np.linspace(0.5, 2.0, m) + 1.0}[ys_kind]

    def run(s):
        c = s.ctx
        src = s.sources(n)  # uploaded before any fill: an upload stores pending fills
        dst = [garbage(c, n, j) for j in range(m)]
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer_scaled(al, src[:k], xs_scale, dst, ys_scale)
        got = [v.numpy() for v in dst]
        for v in dst:
            v.free()
        return got

    got, dl, el = both(sides, run)
    if ys_kind == "scaled":  # 0 * ys is still +0.0, but the call is not the fill + gemm_outer pair: not consumed
        assert calls(dl, "fill") == m and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + 2 * m)
    else:
        assert calls(dl, "fill") == 0 and dl["gemm_outer"]["bytes"] == 8.0 * n * (k + m)
    xs = [a * v for a, v in zip(xs_scale, host_sources(n)[:k])]  # v * s: the one rounding of an eager scal
    ref = oracle.gemm_outer(al, xs, [np.zeros(n) for _ in range(m)])
    bound = outer_bound(al, xs)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])
