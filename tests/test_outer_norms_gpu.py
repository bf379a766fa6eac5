"""Norms from the deferred gemm_outer (iterative-solver_amd/csrc/outer_norms.h): when the call that
launches a pending gemm_outer record is ssp_dot(y, y, n) on one of its destinations, the launch is the
norm-carrying (NRM) instance of k_gemm_outer, and that dot and the same dot of the record's other
destinations are answered from the sums it left, with no k_dot_partial launch.

Every vector and every dot is compared bit for bit (np.array_equal, and equal sign bits) with the same
calls on a second context created with SSP_DEFER_OUTER=0, which launches every gemm_outer at once and
runs every axpy and dot by itself; a third context, created with SSP_OUTER_NORMS=0, defers but keeps no
norms.  Each dot is also held to the norm of the downloaded vector at n eps |y|^2, the bound of a sum of
n non-negative terms in any order.

The ledger tells the paths apart: a served dot opens no row, so a chain whose dots were all served has no
"dot" row, and the record's row is the one tests/test_deferred_outer_gpu.py pins (one call,
8 n (k + m + e) bytes for e attached terms).  The NRM instance exists for up to 8 destinations; a wider
record declines and every dot runs as before (m "dot" calls).

Shapes, each for one tail path of the dot's walk (windows of 256 double2 = 512 doubles per wave):
  2049        4 whole windows plus the odd element
  2248        even, 100 positions past the last whole window
  4099        1 such position plus the odd element
  70001       184 positions plus the odd element, 34 workgroups
  4264305     (4194304 + 70001) a wave's second grid-stride visit: 8192 waves cover 4194304 doubles
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_distributed import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
NS = [2049, 2248, 4099, 70001]
MS = [1, 2, 3, 4, 8, 16]
KS = [1, 5, 48]
KMAX = max(KS)
NBIG = 4_194_304 + 70_001
NRM_MAX = 8  # destinations of the widest norm-carrying instance


def built(m):
    return m <= NRM_MAX


_host = {}


def host_sources(n, k=KMAX):
    if n not in _host:
        r = np.random.default_rng(n)
        _host[n] = [r.uniform(-1, 1, n) for _ in range(k)]
    return _host[n]


def host_x(n, j):
    return np.random.default_rng(9000 + 31 * j + n).uniform(-1, 1, n)


def coef(k, m):
    return np.random.default_rng(1000 * k + m).uniform(-1, 1, (k, m))


def lam(m):
    return -np.random.default_rng(m).uniform(0.5, 2, m)


ATTACH = {"all": lambda j: True, "subset": lambda j: j % 3 != 1, "none": lambda j: False}


class Side:
    """One context with the sources of every n uploaded once."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.src = {}

    def sources(self, n, k=KMAX):
        if n not in self.src:
            self.src[n] = [self.ctx.upload(v) for v in host_sources(n, k)]
        return self.src[n]

    def drop(self, n):
        for v in self.src.pop(n, []):
            v.free()


def make_context(**env):
    import subspace_hip as sh

    names = ("SSP_DEFER_OUTER", "SSP_OUTER_NORMS")
    old = {k: os.environ.pop(k, None) for k in names}
    try:
        os.environ.update(env)
        ctx = sh.Context(0)
    finally:
        for k in names:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    ctx.ledger_enable(True)
    return ctx


@pytest.fixture(scope="module")
def sides():
    import subspace_hip as sh

    if sh.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X")
    norms, eager = make_context(), make_context(SSP_DEFER_OUTER="0")
    yield Side(norms), Side(eager)
    norms.close()
    eager.close()


@pytest.fixture(scope="module")
def switched_off():
    ctx = make_context(SSP_OUTER_NORMS="0")
    yield Side(ctx)
    ctx.close()


def garbage(ctx, n, seed=0):
    """A vector that holds data, so that a destination read instead of overwritten shows."""
    return ctx.upload(np.random.default_rng(77 + seed).uniform(1, 2, n))


def view(ctx, v, off, n):
    import subspace_hip as sh

    return sh.DeviceVector(ctx, n, v.ptr + 8 * off, owner=False)


def both(sides, fn):
    """fn(side) -> arrays on each context, which must all agree bit for bit.  Returns the first side's
    arrays and every ledger."""
    out = []
    for s in sides:
        s.ctx.ledger_reset()
        arrays = fn(s)
        out.append(([np.asarray(a) for a in arrays], s.ctx.ledger()))
    first = out[0][0]
    for arrays, _ in out[1:]:
        assert len(first) == len(arrays)
        for a, b in zip(first, arrays):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
            assert np.array_equal(np.signbit(a), np.signbit(b))  # array_equal takes -0.0 for +0.0
    return [first] + [ledger for _, ledger in out]


def calls(ledger, op):
    return ledger.get(op, {"calls": 0})["calls"]


def check_record_row(ledger, row, n, k, m, e):
    assert calls(ledger, row) == 1 and ledger[row]["bytes"] == 8.0 * n * (k + m + e)


def check_dots(vectors, dots):
    """Each dot against the downloaded vector: a sum of n non-negative terms, in any order."""
    for v, d in zip(vectors, dots):
        ref = float(np.dot(v, v))
        assert abs(d - ref) <= v.size * EPS * ref


def start_chain(s, n, m, k, al, attach="all", set_form=False):
    """fill x m + gemm_outer (or gemm_outer_set), then y_j += a_j x_j for the chosen j: the record is
    pending, with its terms, when this returns.  -> (dst, own)"""
    c = s.ctx
    src = s.sources(n)  # every vector exists before the gemm_outer: an upload launches the record
    dst = [garbage(c, n, j) for j in range(m)]
    own = [c.upload(host_x(n, j)) for j in range(m)]
    a = lam(m)
    c.ledger_reset()
    if set_form:
        c.gemm_outer_set(al, src[:k], dst)
    else:
        for v in dst:
            c.fill(0.0, v)
        c.gemm_outer(al, src[:k], dst)
    for j in range(m):
        if ATTACH[attach](j):
            c.axpy(a[j], own[j], dst[j])
    return dst, own


def finish(dst, own, dots, extra=()):
    got = [v.numpy() for v in dst]
    for v in dst + own:
        v.free()
    return got + [np.asarray(dots, dtype=np.float64)] + list(extra)


def run_chain(s, n, m, k, al, attach="all", set_form=False):
    dst, own = start_chain(s, n, m, k, al, attach, set_form)
    dots = [s.ctx.dot(v, v) for v in dst]
    return finish(dst, own, dots)


def terms(m, k, attach):
    """Attached terms on the deferring side: none when the epilogue sources do not fit behind k."""
    return sum(ATTACH[attach](j) for j in range(m)) if k + m <= 64 else 0


# 1. the headline's own chain: every shape, both forms, every attachment
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_chain_dots_are_the_eager_dots(sides, n, m, k):
    al = coef(k, m)
    for set_form in (False, True):
        row = "gemm_outer_set" if set_form else "gemm_outer"
        for attach in ATTACH:
            got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al, attach, set_form))
            e = terms(m, k, attach)
            check_record_row(dl, row, n, k, m, e)
            assert calls(dl, "axpy") == 0 and calls(el, "axpy") == e
            assert calls(dl, "dot") == (0 if built(m) else m), (set_form, attach)
            assert calls(el, "dot") == m and calls(dl, "fill") == 0
            check_dots(got[:m], got[m])


# 2. a wave's second grid-stride visit
def test_second_grid_stride_visit(sides):
    n, m, k = NBIG, 2, 4
    al = coef(k, m)
    for s in sides:
        s.sources(n, k)
    try:
        got, dl, el = both(sides, lambda s: run_chain(s, n, m, k, al))
    finally:
        for s in sides:
            s.drop(n)
    check_record_row(dl, "gemm_outer", n, k, m, m)
    assert calls(dl, "dot") == 0 and calls(el, "dot") == m
    check_dots(got[:m], got[m])


# 3. the same destination asked twice is served twice, in any order
def test_repeated_and_reordered_queries(sides):
    n, m, k = 4099, 4, 5
    al = coef(k, m)
    order = [2, 0, 2, 3, 1, 1, 0]

    def run(s):
        dst, own = start_chain(s, n, m, k, al)
        return finish(dst, own, [s.ctx.dot(dst[j], dst[j]) for j in order])

    got, dl, el = both(sides, run)
    check_record_row(dl, "gemm_outer", n, k, m, m)
    assert calls(dl, "dot") == 0 and calls(el, "dot") == len(order)
    check_dots([got[j] for j in order], got[m])


# 4. ssp_dot_scaled with unit scales is the same call (decided by value)
def test_dot_scaled_with_unit_scales_is_served(sides):
    n, m, k = 2248, 3, 5
    al = coef(k, m)

    def run(s):
        dst, own = start_chain(s, n, m, k, al)
        return finish(dst, own, [s.ctx.dot_scaled(v, 1.0, v, 1.0) for v in dst])

    got, dl, el = both(sides, run)
    assert calls(dl, "dot") == 0 and calls(el, "dot") == m
    check_dots(got[:m], got[m])


# 5. calls that are not the norm of a destination: correct values, and the later dots run as they always did
NOT_SERVED = ["dot_xy", "offset_view", "shorter_view", "dot_scaled", "non_destination", "synchronize", "download",
              "copy"]


@pytest.mark.parametrize("what", NOT_SERVED)
def test_not_served(sides, what):
    n, m, k = 4099, 3, 5
    al = coef(k, m)

    def run(s):
        c = s.ctx
        scratch = garbage(c, n, 60)
        dst, own = start_chain(s, n, m, k, al)
        first, ndots = [], 1
        if what == "dot_xy":
            first = [c.dot(dst[0], dst[1])]
        elif what == "offset_view":
            w = view(c, dst[1], 2, n - 2)
            first = [c.dot(w, w)]
        elif what == "shorter_view":
            w = view(c, dst[1], 0, n - 1)
            first = [c.dot(w, w)]
        elif what == "dot_scaled":
            first = [c.dot_scaled(dst[0], 0.5, dst[0], 0.5), c.dot_scaled(dst[0], 1.0, dst[0], 2.0)]
            ndots = 2
        elif what == "non_destination":
            first = [c.dot(s.sources(n)[0], s.sources(n)[0])]
        elif what == "synchronize":
            c.synchronize()
            ndots = 0
        elif what == "download":
            first = [dst[0].numpy()[:8].copy()]
            ndots = 0
        else:
            c.copy(scratch, s.sources(n)[0])
            ndots = 0
        dots = [c.dot(v, v) for v in dst]
        scratch.free()
        return finish(dst, own, dots, [np.ravel(f) for f in first]) + [np.array([ndots])]

    got, dl, el = both(sides, run)
    ndots = int(got[-1][0])
    check_record_row(dl, "gemm_outer", n, k, m, m)
    assert calls(dl, "dot") == m + ndots and calls(el, "dot") == m + ndots
    check_dots(got[:m], got[m])


# 6. after the first served dot, anything that may change a vector makes its next dot a fresh one
@pytest.mark.parametrize("what", ["axpy", "scal", "upload", "fill", "free_realloc"])
def test_invalidation(sides, what):
    n, m, k = 70001, 3, 5
    al = coef(k, m)
    fresh = host_x(n, 40)

    def run(s):
        c = s.ctx
        dst, own = start_chain(s, n, m, k, al)
        d0 = c.dot(dst[0], dst[0])
        if what == "axpy":
            c.axpy(0.75, own[0], dst[1])
        elif what == "scal":
            c.scal(-1.5, dst[1])
        elif what == "upload":
            c.upload_into(dst[1], fresh)
        elif what == "fill":
            c.fill(0.0, dst[1])
        else:
            ptr = dst[1].ptr
            dst[1].free()
            held = []  # the arena hands out its cached blocks of this size oldest first
            for _ in range(512):
                v = c.alloc(n)
                if v.ptr == ptr:
                    break
                held.append(v)
            assert v.ptr == ptr  # the same address and n, new data
            c.upload_into(v, fresh)
            dst[1] = v
            for h in held:
                h.free()
        dots = [d0] + [c.dot(v, v) for v in dst[1:]]
        return finish(dst, own, dots)

    got, dl, el = both(sides, run)
    check_record_row(dl, "gemm_outer", n, k, m, m)
    assert calls(dl, "dot") == m - 1 and calls(el, "dot") == m  # only the first was served
    check_dots(got[:m], got[m])
    if what == "fill":
        assert got[m][1] == 0.0
    if what in ("upload", "free_realloc"):
        assert np.array_equal(got[1], fresh)


# 7. an infinite element reaches the norm of its own destination only
def test_infinite_element(sides):
    n, m, k = 4099, 3, 5
    al = coef(k, m)
    xinf = host_x(n, 0).copy()
    xinf[[0, 511, 2048, n - 1]] = [np.inf, -np.inf, np.inf, -np.inf]

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
        dots = [c.dot(v, v) for v in dst]
        return finish(dst, [x], dots)

    got, dl, el = both(sides, run)
    check_record_row(dl, "gemm_outer", n, k, m, 1)
    assert calls(dl, "dot") == 0 and calls(el, "dot") == m
    assert np.isinf(got[m][1]) and got[m][1] > 0
    assert np.isfinite(got[m][0]) and np.isfinite(got[m][2])


# 8. SSP_OUTER_NORMS=0: the same bits, every dot by itself
@pytest.mark.parametrize("n,m,k", [(2049, 1, 1), (2248, 3, 5), (4099, 8, 48), (70001, 4, 48)])
def test_switch(sides, switched_off, n, m, k):
    al = coef(k, m)
    got, dl, ol, el = both((sides[0], switched_off, sides[1]), lambda s: run_chain(s, n, m, k, al))
    for ledger in (dl, ol):
        check_record_row(ledger, "gemm_outer", n, k, m, m)
    assert calls(dl, "dot") == 0 and calls(ol, "dot") == m and calls(el, "dot") == m


# 9. two ranks on one device over the host hub: each served dot reduces its own rank-local sum
def test_two_ranks():
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", SSP_HUB_PORT=str(port))
        env.pop("SSP_OUTER_NORMS", None)
        env.pop("SSP_DEFER_OUTER", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "outer_norms_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "outer_norms OK" in out, f"rank {rank} failed:\n{out[-4000:]}"
