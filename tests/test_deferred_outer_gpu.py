"""Deferred gemm_outer (iterative-solver_amd/csrc/pending_outer.h): a write-only ssp_gemm_outer of one
launch is recorded, not launched, and an ssp_axpy onto one of its destinations becomes an epilogue term
of that launch (the EPI instance of k_gemm_outer) instead of a pass of its own.

Every result is compared bit for bit (np.array_equal, and equal sign bits) with the same calls on a
second context created with SSP_DEFER_OUTER=0, which launches every gemm_outer at once and every axpy
by itself.  The fused cases are also held to the oracle at the bound tests/test_ops_gpu.py::test_gemm_outer
uses, with the axpy counted as one more source of the sum: |got - oracle| <= 4 (k + 1) eps
(sum_i |alpha_i| |x_i| + |a| |x|).  Destinations and x vectors hold random data first.

The ledger tells the paths apart: a fused chain is one "gemm_outer" call of 8 n (k + m + e) bytes for
e attached terms and no "axpy" row; otherwise the "axpy" rows are there.

Shapes: n just above the exact-mode limit (2048), odd tails, whole and part wave windows of 512
doubles; m across the kernel's instances up to kOuterDst = 16; k across the 4-source groups, their
remainder and kOuterSrc = 64; k + m on both sides of the epilogue's fit limit (k + m <= 64).
"""
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NS = [2049, 2560, 4099, 70001]
MS = [1, 3, 8, 16]
KS = [1, 4, 5, 48, 64]
KMAX = max(KS)


def fits(k, m):
    return k + m <= 64


_host = {}


def host_sources(n):
    if n not in _host:
        r = np.random.default_rng(n)
        _host[n] = [r.uniform(-1, 1, n) for _ in range(KMAX)]
    return _host[n]


def host_x(n, j):
    return np.random.default_rng(9000 + 31 * j + n).uniform(-1, 1, n)


def coef(k, m):
    return np.random.default_rng(1000 * k + m).uniform(-1, 1, (k, m))


def lam(m):
    return -np.random.default_rng(m).uniform(0.5, 2, m)


class Side:
    """One context with the sources of every n uploaded once."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.src = {}

    def sources(self, n):
        if n not in self.src:
            self.src[n] = [self.ctx.upload(v) for v in host_sources(n)]
        return self.src[n]


@pytest.fixture(scope="module")
def sides():
    import subspace_hip as sh

    if sh.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X")
    old = os.environ.pop("SSP_DEFER_OUTER", None)
    try:
        deferred = sh.Context(0)
        os.environ["SSP_DEFER_OUTER"] = "0"
        eager = sh.Context(0)
    finally:
        os.environ.pop("SSP_DEFER_OUTER", None)
        if old is not None:
            os.environ["SSP_DEFER_OUTER"] = old
    for c in (deferred, eager):
        c.ledger_enable(True)
    yield Side(deferred), Side(eager)
    deferred.close()
    eager.close()


def garbage(ctx, n, seed=0):
    """A vector that holds data, so that a destination read instead of overwritten shows."""
    return ctx.upload(np.random.default_rng(77 + seed).uniform(1, 2, n))


def view(ctx, v, off, n):
    import subspace_hip as sh

    return sh.DeviceVector(ctx, n, v.ptr + 8 * off, owner=False)


def both(sides, fn):
    """fn(side) -> arrays on the deferring and on the eager context, which must agree bit for bit.
    Returns the deferring side's arrays and both ledgers."""
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


def fused_bound(al, xs, a, x):
    """The gemm_outer bound of tests/test_ops_gpu.py with the attached axpy as source k + 1."""
    k = al.shape[0]
    return 4 * (k + 1) * EPS * (np.abs(al).T @ np.abs(np.array(xs)) + np.abs(np.array(a))[:, None] * np.abs(np.array(x)))


def oracle_chain(al, xs, a, x):
    m = al.shape[1]
    y = oracle.gemm_outer(al, xs, [np.zeros(xs[0].size) for _ in range(m)])
    return [oracle.axpy(a[j], x[j], y[j]) if a[j] is not None else y[j] for j in range(m)]


def check_ledger(dl, el, n, k, m, e, eager_axpy, row="gemm_outer", rest=0):
    """Deferring side: one `row` call carrying e terms and `rest` separate axpy calls; eager side: the
    plain write-only call and every axpy by itself."""
    assert calls(dl, row) == 1 and dl[row]["bytes"] == 8.0 * n * (k + m + e)
    assert calls(dl, "axpy") == rest
    assert calls(el, row) == 1 and el[row]["bytes"] == 8.0 * n * (k + m)
    assert calls(el, "axpy") == eager_axpy


def run_chain(s, n, m, k, al, a, set_form=False, xvecs=None, between=None):
    """fill x m + gemm_outer (or gemm_outer_set), then y_j += a_j x_j for every j with a term, then the
    norm of every destination.  xvecs(ctx, src, dst) -> the x vectors; between(ctx, src, dst) runs
    after the gemm_outer."""
    c = s.ctx
    src = s.sources(n)  # every vector exists before the gemm_outer: an upload launches the record
    dst = [garbage(c, n, j) for j in range(m)]
    own = [c.upload(host_x(n, j)) for j in range(m)]
    xs = xvecs(c, src, dst, own) if xvecs else own
    c.ledger_reset()
    if set_form:
        c.gemm_outer_set(al, src[:k], dst)
    else:
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src[:k], dst)
    if between:
        between(c, src, dst)
    for j in range(m):
        if a[j] is not None:
            c.axpy(a[j], xs[j], dst[j])
    dots = np.array([c.dot(v, v) for v in dst])
    got = [v.numpy() for v in dst]
    for v in dst + own:
        v.free()
    return got + [dots]


# 1. the headline's own chain, every shape
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_fill_gemm_outer_axpy_dot_chain(sides, n, m, k):
    al, a = coef(k, m), list(lam(m))
    got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al, a))
    if fits(k, m):
        check_ledger(dl, el, n, k, m, m, m)
    else:
        check_ledger(dl, el, n, k, m, 0, m, rest=m)
    assert calls(dl, "fill") == 0 and "gemm_outer_set" not in dl
    xs, x = host_sources(n)[:k], [host_x(n, j) for j in range(m)]
    ref, bound = oracle_chain(al, xs, a, x), fused_bound(al, xs, a, x)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 2. the same chain from gemm_outer_set
@pytest.mark.parametrize("n,m,k", [(2049, 1, 1), (2560, 3, 5), (4099, 8, 48), (70001, 16, 48), (70001, 2, 64)])
def test_gemm_outer_set_axpy_dot_chain(sides, n, m, k):
    al, a = coef(k, m), list(lam(m))
    got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al, a, set_form=True))
    if fits(k, m):
        check_ledger(dl, el, n, k, m, m, m, row="gemm_outer_set")
    else:
        check_ledger(dl, el, n, k, m, 0, m, row="gemm_outer_set", rest=m)
    assert "gemm_outer" not in dl  # the row keeps the name of the call made
    xs, x = host_sources(n)[:k], [host_x(n, j) for j in range(m)]
    ref, bound = oracle_chain(al, xs, a, x), fused_bound(al, xs, a, x)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 3. k + m on each side of the fit limit, for both destination widths that reach it
@pytest.mark.parametrize("k,m,fused", [(56, 8, True), (57, 8, False), (48, 16, True), (49, 16, False)])
def test_epilogue_fit_limit(sides, k, m, fused):
    n = 4099
    al, a = coef(k, m), list(lam(m))
    got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al, a))
    assert fits(k, m) == fused
    check_ledger(dl, el, n, k, m, m if fused else 0, m, rest=0 if fused else m)
    xs, x = host_sources(n)[:k], [host_x(n, j) for j in range(m)]
    ref, bound = oracle_chain(al, xs, a, x), fused_bound(al, xs, a, x)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 4. terms on some destinations only
@pytest.mark.parametrize("n,m,k", [(2049, 3, 5), (4099, 8, 48), (70001, 16, 4)])
def test_axpy_on_a_subset_of_the_destinations(sides, n, m, k):
    al = coef(k, m)
    a = [v if j % 3 != 1 else None for j, v in enumerate(lam(m))]
    e = sum(v is not None for v in a)
    got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al, a))
    check_ledger(dl, el, n, k, m, e, e)
    xs, x = host_sources(n)[:k], [host_x(n, j) for j in range(m)]
    ref = oracle_chain(al, xs, a, x)
    bound = fused_bound(al, xs, [v or 0.0 for v in a], x)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 5. a second axpy on one destination launches the record and runs by itself
def test_two_axpys_on_one_destination(sides):
    n, m, k = 4099, 3, 5
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)
        dst = [garbage(c, n, j) for j in range(m)]
        x = [c.upload(host_x(n, j)) for j in range(2)]
        c.ledger_reset()
        c.gemm_outer_set(al, src[:k], dst)
        c.axpy(0.75, x[0], dst[1])
        c.axpy(-1.5, x[1], dst[1])
        got = [v.numpy() for v in dst]
        for v in dst + x:
            v.free()
        return got

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 1, 2, row="gemm_outer_set", rest=1)
    xs = host_sources(n)[:k]
    y = oracle.gemm_outer(al, xs, [np.zeros(n) for _ in range(m)])
    ref = oracle.axpy(-1.5, host_x(n, 1), oracle.axpy(0.75, host_x(n, 0), y[1]))
    bound = 4 * (k + 2) * EPS * (np.abs(al[:, 1]) @ np.abs(np.array(xs)) + 0.75 * np.abs(host_x(n, 0)) + 1.5 * np.abs(host_x(n, 1)))
    assert np.all(np.abs(got[1] - ref) <= bound)


# 6. zero coefficients: a sum that is exactly -0.0 keeps its sign where no term is attached, and takes
#    the sign the separate axpy gives it where one is
@pytest.mark.parametrize("n", [2049, 4099])
def test_zero_coefficients_and_negative_zero_sums(sides, n):
    m, k = 4, 2
    tiny = np.full(n, 1e-200)
    al = np.full((k, m), -1e-200)  # every product underflows to -0.0: fma(al, x, +0.0) = -0.0

    def run(s):
        c = s.ctx
        src = [c.upload(tiny) for _ in range(k)]
        dst = [garbage(c, n, j) for j in range(m)]
        x = [c.upload(host_x(n, j)) for j in range(m)]
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src, dst)
        c.axpy(0.0, x[0], dst[0])
        c.axpy(-0.0, x[1], dst[1])
        c.axpy(0.0, src[0], dst[2])  # +0.0 * 1e-200 = +0.0
        got = [v.numpy() for v in dst]
        for v in dst + x + src:
            v.free()
        return got

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 3, 3)
    assert all(np.all(g == 0.0) for g in got)
    assert np.all(np.signbit(got[3]))  # no term: the -0.0 sum is stored as it is
    assert not np.any(np.signbit(got[2]))  # -0.0 + (+0.0) = +0.0
    x0, x1 = host_x(n, 0), host_x(n, 1)
    assert np.array_equal(np.signbit(got[0]), x0 < 0)  # 0.0 * x0 is -0.0 where x0 < 0, and -0.0 + -0.0 = -0.0
    assert np.array_equal(np.signbit(got[1]), x1 > 0)


# 7. an infinite x reaches its own destination only
def test_infinite_x_touches_only_its_destination(sides):
    n, m, k = 4099, 3, 5
    al = coef(k, m)
    xinf = host_x(n, 0).copy()
    xinf[[0, 511, 512, 2048, n - 1]] = [np.inf, -np.inf, np.inf, -np.inf, np.inf]

    def run(s):
        c = s.ctx
        src = s.sources(n)
        dst = [garbage(c, n, j) for j in range(m)]
        x = c.upload(xinf)
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src[:k], dst)
        c.axpy(0.5, x, dst[1])
        got = [v.numpy() for v in dst]
        for v in dst + [x]:
            v.free()
        return got

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 1, 1)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))
    assert np.array_equal(np.isinf(got[1]), np.isinf(xinf)) and not np.any(np.isnan(got[1]))


# 8. x that is a source of the record: attached
def test_x_equal_to_a_source(sides):
    n, m, k = 70001, 8, 48
    al, a = coef(k, m), list(lam(m))
    got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al, a, xvecs=lambda c, src, dst, own: [src[j] for j in range(m)]))
    check_ledger(dl, el, n, k, m, m, m)
    xs = host_sources(n)[:k]
    ref, bound = oracle_chain(al, xs, a, xs[:m]), fused_bound(al, xs, a, xs[:m])
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])


# 9. x that is another destination: its finished value is needed, so the record is launched first
def test_x_equal_to_another_destination(sides):
    n, m, k = 4099, 3, 5
    al = coef(k, m)
    a = [None, -1.25, None]
    got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al, a, xvecs=lambda c, src, dst, own: [None, dst[0], None]))
    check_ledger(dl, el, n, k, m, 0, 1, rest=1)
    xs = host_sources(n)[:k]
    y = oracle.gemm_outer(al, xs, [np.zeros(n) for _ in range(m)])
    assert np.all(np.abs(got[1] - oracle.axpy(-1.25, y[0], y[1])) <= 8 * (k + 1) * EPS * (np.abs(al).T @ np.abs(np.array(xs))).sum(0))


# 10. x zero-filled just before, over garbage: the pending fill of x is stored before the launch reads it
def test_x_with_a_pending_zero_fill(sides):
    n, m, k = 2560, 3, 4
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)
        dst = [garbage(c, n, j) for j in range(m)]
        x = garbage(c, n, 50)
        c.ledger_reset()
        c.fill(0.0, x)
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src[:k], dst)
        c.axpy(3.0, x, dst[2])
        got = [v.numpy() for v in dst] + [x.numpy()]
        for v in dst + [x]:
            v.free()
        return got

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 1, 1)
    assert calls(dl, "fill") == 1 and np.all(got[3] == 0.0)
    ref = oracle.gemm_outer(al, host_sources(n)[:k], [np.zeros(n) for _ in range(m)])
    assert np.all(np.abs(got[2] - ref[2]) <= 4 * k * EPS * (np.abs(al[:, 2]) @ np.abs(np.array(host_sources(n)[:k]))))


# 11. y that is not exactly a destination: an offset view, or the destination with a shorter n
@pytest.mark.parametrize("off,cut", [(2, 0), (0, 2), (0, 1)])
def test_y_as_a_view_of_a_destination_is_not_attached(sides, off, cut):
    n, m, k = 4099, 3, 5
    al = coef(k, m)
    ny = n - off - cut

    def run(s):
        c = s.ctx
        src = s.sources(n)
        dst = [garbage(c, n, j) for j in range(m)]
        x = c.upload(host_x(n, 0))
        c.ledger_reset()
        c.gemm_outer_set(al, src[:k], dst)
        c.axpy(0.5, view(c, x, 0, ny), view(c, dst[1], off, ny))
        got = [v.numpy() for v in dst]
        for v in dst + [x]:
            v.free()
        return got

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 0, 1, row="gemm_outer_set", rest=1)
    y = oracle.gemm_outer(al, host_sources(n)[:k], [np.zeros(n) for _ in range(m)])
    assert np.array_equal(got[1][:off], y[1][:off]) and np.array_equal(got[1][off + ny:], y[1][off + ny:])


# 12. ssp_axpy_scaled: attached with unit scales (decided by value), launched by itself otherwise
@pytest.mark.parametrize("xs,ys,fused", [(1.0, 1.0, True), (0.5, 1.0, False), (1.0, 2.0, False)])
def test_axpy_scaled(sides, xs, ys, fused):
    n, m, k = 4099, 3, 5
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)
        dst = [garbage(c, n, j) for j in range(m)]
        x = c.upload(host_x(n, 0))
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src[:k], dst)
        c.axpy_scaled(-0.75, x, xs, dst[0], ys)
        got = [v.numpy() for v in dst]
        for v in dst + [x]:
            v.free()
        return got

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 1 if fused else 0, 1, rest=0 if fused else 1)


# 13. anything else between the gemm_outer and the axpy launches the record
@pytest.mark.parametrize("what", ["download", "synchronize", "copy", "gemm_outer"])
def test_an_entry_point_in_between_launches_the_record(sides, what):
    n, m, k = 4099, 3, 5
    al, al2 = coef(k, m), coef(k, 2)
    extra = []

    def between(c, src, dst):
        if what == "download":
            extra.append(dst[0].numpy())
        elif what == "synchronize":
            c.synchronize()
        elif what == "copy":
            c.copy(c._scratch[0], src[0])
        else:
            c.gemm_outer_set(al2, src[:k], c._scratch)

    def run(s):
        c = s.ctx
        c._scratch = [garbage(c, n, 60 + j) for j in range(2)]
        out = run_chain(s, n, m, k, al, list(lam(m)), between=between)
        out += [v.numpy() for v in c._scratch]
        for v in c._scratch:
            v.free()
        return out

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 0, m, rest=m)
    if what == "download":
        assert np.array_equal(extra[0], extra[1])
    if what == "gemm_outer":  # the second record took no term either: no axpy named its destinations
        assert calls(dl, "gemm_outer_set") == 1 and dl["gemm_outer_set"]["bytes"] == 8.0 * n * (k + 2)


# 14. x freed before anything else launches the record: the free does, so the block is read before reuse
def test_free_of_x_launches_the_record_first(sides):
    n, m, k = 70001, 3, 5
    al = coef(k, m)

    def run(s):
        c = s.ctx
        src = s.sources(n)
        dst = [garbage(c, n, j) for j in range(m)]
        x = c.upload(host_x(n, 0))
        c.ledger_reset()
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src[:k], dst)
        c.axpy(-2.0, x, dst[0])
        x.free()
        again = garbage(c, n, 70)  # recycles x's block, after the launch that read it was queued
        got = [v.numpy() for v in dst]
        for v in dst + [again]:
            v.free()
        return got

    got, dl, el = both(sides, run)
    check_ledger(dl, el, n, k, m, 1, 1)
    xs = host_sources(n)[:k]
    a, x = [-2.0, None, None], [host_x(n, 0)] * m
    ref, bound = oracle_chain(al, xs, a, x), fused_bound(al, xs, [-2.0, 0.0, 0.0], x)
    for j in range(m):
        assert np.all(np.abs(got[j] - ref[j]) <= bound[j])
