"""Both solution constructions of a step in one launch (OuterPair in iterative-solver_amd/csrc/pending_outer.h,
k_gemm_outer_pair in kernels_outer.hip): two gemm_outers of the same kind, shape and alphas stay pending as a
pair, the ssp_axpy of the first one's destination j onto the second one's destination j becomes a register
term, and the ssp_dot(y, y) of a destination of the second launches both as one norm-carrying kernel.

Every vector and every dot is compared bit for bit (np.array_equal with NaNs equal, and equal sign bits)
across three contexts: the default one, one created with SSP_DEFER_OUTER=0 (eager: every gemm_outer, axpy and
dot by itself) and one created with SSP_OUTER_PAIR=0 (defers, never pairs: the rows of before the pair).
Each dot is also held to the norm of the downloaded vector at n eps |y|^2, the bound of a sum of n
non-negative terms in any order.

The ledger tells the paths apart.  All contexts are created with SSP_LEDGER_DETAIL, so the pair's launch shows
as "gemm_outer [pair<M,1> kxm regE nrm]" (or gemm_outer_set): one row, two calls, 8 n (2 k + 2 m) bytes, no
"axpy" and no "dot" row.  Whatever un-pairs or prevents pairing must show exactly the rows of the
SSP_OUTER_PAIR=0 context.  Rows are summed over their detail tags for the counts.

Shapes, each for one tail path of the dot's walk (windows of 256 double2 = 512 doubles per wave; the pair's
kernel covers each as two halves of 128 double2):
  2049        4 whole windows plus the odd element
  2248        even, 100 positions past the last whole window
  4099        1 such position plus the odd element
  70001       184 positions plus the odd element, 34 workgroups
  4264305     (4194304 + 70001) a wave's second grid-stride visit: 8192 waves cover 4194304 doubles
k = 13 gives whole source groups plus a remainder for groups of 4 and of 8 sources.
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
KS = [1, 5, 13, 48]
KMAX = max(KS)
NBIG = 4_194_304 + 70_001
PAIR_MAX = 8  # destinations of the widest pair kernel (and of the widest norm-carrying instance)
ENV = ("SSP_DEFER_OUTER", "SSP_OUTER_NORMS", "SSP_OUTER_PAIR", "SSP_LEDGER_DETAIL")

_host = {}


def host_sources(n, space):
    """The k sources of one space (0: the first call's, 1: the second call's) at length n, made once."""
    if (n, space) not in _host:
        r = np.random.default_rng(2 * n + space)
        _host[n, space] = [r.uniform(-1, 1, n) for _ in range(KMAX)]
    return _host[n, space]


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

    def sources(self, n, space, k=KMAX):
        if (n, space) not in self.src:
            self.src[n, space] = [self.ctx.upload(v) for v in host_sources(n, space)[:k]]
        return self.src[n, space]

    def drop(self, n):
        for space in (0, 1):
            for v in self.src.pop((n, space), []):
                v.free()


def make_context(**env):
    import subspace_hip as sh

    old = {k: os.environ.pop(k, None) for k in ENV}
    try:
        os.environ.update(env)
        os.environ["SSP_LEDGER_DETAIL"] = "1"
        ctx = sh.Context(0)
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    ctx.ledger_enable(True)
    return ctx


@pytest.fixture(scope="module")
def sides():
    """(default, eager, never pairs)"""
    import subspace_hip as sh

    if sh.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X")
    ctxs = [make_context(), make_context(SSP_DEFER_OUTER="0"), make_context(SSP_OUTER_PAIR="0")]
    yield tuple(Side(c) for c in ctxs)
    for c in ctxs:
        c.close()


def garbage(ctx, n, seed=0):
    """A vector that holds data, so that a destination read instead of overwritten shows."""
    return ctx.upload(np.random.default_rng(77 + seed).uniform(1, 2, n))


def view(ctx, v, off, n):
    import subspace_hip as sh

    return sh.DeviceVector(ctx, n, v.ptr + 8 * off, owner=False)


def three(sides, fn):
    """fn(side) -> arrays on each context, which must all agree bit for bit.  Returns the first side's arrays
    and the three ledgers (default, eager, never pairs)."""
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


def rows(ledger):
    """{op: (calls, bytes)} summed over the detail tags."""
    out = {}
    for name, e in ledger.items():
        op = name.split(" [")[0]
        c, b = out.get(op, (0, 0.0))
        out[op] = (c + e["calls"], b + e["bytes"])
    return {op: v for op, v in out.items() if v[0]}


def calls(ledger, op):
    return rows(ledger).get(op, (0, 0.0))[0]


def pair_launches(ledger):
    c = sum(e["calls"] for name, e in ledger.items() if "[pair<" in name)
    assert c % 2 == 0
    return c // 2


def check_pair_row(ledger, row, n, k, m, e):
    """One launch: one detail row under the calls' own name, two calls, the bytes of both constructions."""
    tagged = [name for name in ledger if "[pair<" in name and ledger[name]["calls"]]
    assert len(tagged) == 1 and tagged[0].startswith(row + " [") and f"reg{e} nrm" in tagged[0], list(ledger)
    assert rows(ledger)[row] == (2, 8.0 * n * (2 * k + 2 * m))
    assert calls(ledger, "axpy") == 0 and calls(ledger, "dot") == 0 and calls(ledger, "fill") == 0


def check_dots(vectors, dots):
    """Each dot against the downloaded vector: a sum of n non-negative terms, in any order."""
    for v, d in zip(vectors, dots):
        ref = float(np.dot(v, v))
        assert abs(d - ref) <= v.size * EPS * ref


class Chain:
    """The vectors of one run of the headline chain on one context: everything exists before the first
    gemm_outer (an upload launches the pending records)."""

    def __init__(self, s, n, m, k, nextra=0):
        c = self.ctx = s.ctx
        self.n, self.m, self.k = n, m, k
        self.sp, self.sa = list(s.sources(n, 0)[:k]), list(s.sources(n, 1)[:k])
        self.dp = [garbage(c, n, j) for j in range(m)]
        self.da = [garbage(c, n, 20 + j) for j in range(m)]
        self.extra = [c.upload(host_x(n, 50 + j)) for j in range(nextra)]
        self.a = lam(max(m, 1))
        c.ledger_reset()

    def first(self, al, set_form=False):
        c = self.ctx
        if set_form:
            c.gemm_outer_set(al, self.sp, self.dp)
        else:
            for v in self.dp:
                c.fill(0.0, v)
            c.gemm_outer(al, self.sp, self.dp)

    def second(self, al, set_form=False):
        c = self.ctx
        if set_form:
            c.gemm_outer_set(al, self.sa, self.da)
        else:
            for v in self.da:
                c.fill(0.0, v)
            c.gemm_outer(al, self.sa, self.da)

    def axpys(self, attach="all", skip=()):
        for j in range(min(len(self.dp), len(self.da))):
            if ATTACH[attach](j) and j not in skip:
                self.ctx.axpy(self.a[j], self.dp[j], self.da[j])

    def dots(self):
        return [self.ctx.dot(v, v) for v in self.da]

    def finish(self, dots, more=()):
        """-> dp..., da..., dots, more..."""
        got = [v.numpy() for v in self.dp + self.da]
        for v in self.dp + self.da + self.extra:
            v.free()
        return got + [np.asarray(dots, dtype=np.float64)] + [np.ravel(x) for x in more]


def run_chain(s, n, m, k, al, attach="all", set_form=False):
    ch = Chain(s, n, m, k)
    ch.first(al, set_form)
    ch.second(al, set_form)
    ch.axpys(attach)
    return ch.finish(ch.dots())


def nterms(m, attach):
    return sum(ATTACH[attach](j) for j in range(m))


# 1. the headline chain: every shape, both forms, every attachment
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_headline_chain(sides, n, m, k):
    al = coef(k, m)
    for set_form in (False, True):
        row = "gemm_outer_set" if set_form else "gemm_outer"
        for attach in ATTACH:
            got, dl, el, ol = three(sides, lambda s: run_chain(s, n, m, k, al, attach, set_form))
            e = nterms(m, attach)
            if m <= PAIR_MAX:
                assert pair_launches(dl) == 1, (set_form, attach)
                check_pair_row(dl, row, n, k, m, e)
            else:  # 16 destinations decline: the rows of before
                assert pair_launches(dl) == 0 and rows(dl) == rows(ol)
                assert rows(dl)[row] == (2, 8.0 * n * (2 * k + 2 * m + e)) and calls(dl, "dot") == m
            assert pair_launches(ol) == 0 and pair_launches(el) == 0
            assert rows(el)[row] == (2, 8.0 * n * (2 * k + 2 * m))
            assert calls(el, "axpy") == e and calls(el, "dot") == m
            check_dots(got[m:2 * m], got[2 * m])


# a wave's second grid-stride visit
def test_second_grid_stride_visit(sides):
    n, m, k = NBIG, 2, 4
    al = coef(k, m)
    for s in sides:
        for space in (0, 1):
            s.sources(n, space, k)
    try:
        got, dl, el, ol = three(sides, lambda s: run_chain(s, n, m, k, al))
    finally:
        for s in sides:
            s.drop(n)
    assert pair_launches(dl) == 1
    check_pair_row(dl, "gemm_outer", n, k, m, m)
    check_dots(got[m:2 * m], got[2 * m])


# 2. whatever un-pairs or prevents pairing: the rows of before, the eager bits
AFTER = ["axpy_foreign_x", "axpy_other_j", "second_axpy_same_j", "dot_on_first", "download", "synchronize", "copy",
         "fill_over_first_destination", "fill_over_second_source", "scal_of_second_destination"]
BETWEEN = ["fill_over_first_destination", "fill_nonzero", "synchronize"]
SECOND = ["reads_first_destination", "writes_first_source", "alpha_one_bit", "alpha_zero_sign", "k", "m", "n",
          "set_after_rmw", "rmw_after_set"]
NOT_PAIRED = [("after", w) for w in AFTER] + [("between", w) for w in BETWEEN] + [("second", w) for w in SECOND]


@pytest.mark.parametrize("where,what", NOT_PAIRED)
def test_not_paired(sides, where, what):
    n, m, k = 4099, 3, 5
    al = coef(k, m)
    if what == "alpha_zero_sign":
        al[2, 1] = 0.0
    al2 = al.copy()
    if what == "alpha_one_bit":
        al2.view(np.uint64)[k - 1, m - 1] ^= np.uint64(1)
    elif what == "alpha_zero_sign":
        al2[2, 1] = -0.0

    def run(s):
        c = s.ctx
        ch = Chain(s, n, m, k, nextra=3)
        own, scratch, mine = ch.extra
        owned = ch.dp + ch.da
        more = []
        if what == "reads_first_destination":
            ch.sa[1] = ch.dp[0]
        elif what == "writes_first_source":
            c.copy(mine, ch.sp[k - 1])  # a private last source for the first call
            ch.sp[k - 1] = mine
            ch.da[0] = mine
        elif what == "fill_over_second_source":
            c.copy(mine, ch.sa[0])  # a private first source for the second call
            ch.sa[0] = mine
        elif what == "k":
            ch.sa = ch.sa[:k - 1]
        elif what == "m":
            ch.da = ch.da[:m - 1]
        elif what == "n":
            ch.sa = [view(c, v, 0, n - 1) for v in ch.sa]
            ch.da = [view(c, v, 0, n - 1) for v in ch.da]
        c.ledger_reset()
        ch.first(al, set_form=what == "rmw_after_set")
        if where == "between":
            if what == "fill_over_first_destination":
                c.fill(0.0, ch.dp[0])
            elif what == "fill_nonzero":
                c.fill(1.5, scratch)
            else:
                c.synchronize()
        ch.second(al2[:len(ch.sa), :len(ch.da)], set_form=what == "set_after_rmw")
        if what == "n":
            for j in range(m):
                c.axpy(ch.a[j], view(c, ch.dp[j], 0, n - 1), ch.da[j])
        elif what == "axpy_foreign_x":
            c.axpy(0.75, own, ch.da[0])
            ch.axpys(skip=(0,))
        elif what == "axpy_other_j":
            c.axpy(0.75, ch.dp[1], ch.da[0])
            ch.axpys(skip=(0,))
        else:
            ch.axpys()
        if where == "after":
            if what == "second_axpy_same_j":
                c.axpy(0.75, ch.dp[0], ch.da[0])
            elif what == "dot_on_first":
                more.append(c.dot(ch.dp[0], ch.dp[0]))
            elif what == "download":
                more.append(ch.dp[0].numpy()[:8].copy())
            elif what == "synchronize":
                c.synchronize()
            elif what == "copy":
                c.copy(scratch, ch.sp[0])
            elif what == "fill_over_first_destination":
                c.fill(0.0, ch.dp[1])
            elif what == "fill_over_second_source":
                c.fill(0.0, mine)
            elif what == "scal_of_second_destination":
                c.scal(-1.5, ch.da[0])
        dots = ch.dots()
        got = [v.numpy() for v in ch.dp + ch.da + owned + [scratch, mine]]
        for v in owned + ch.extra:
            v.free()
        return got + [np.asarray(dots, dtype=np.float64)] + [np.ravel(x) for x in more]

    got, dl, el, ol = three(sides, run)
    assert pair_launches(dl) == 0 and pair_launches(ol) == 0
    assert rows(dl) == rows(ol), (rows(dl), rows(ol))


# 3. zero fills that touch no operand keep the pair
@pytest.mark.parametrize("what", ["unrelated_between", "unrelated_after", "second_source_before_its_call"])
def test_fill_that_keeps_the_pair(sides, what):
    n, m, k = 4099, 3, 5
    al = coef(k, m)

    def run(s):
        c = s.ctx
        ch = Chain(s, n, m, k, nextra=2)
        other, mine = ch.extra
        if what == "second_source_before_its_call":
            c.copy(mine, ch.sa[2])
            ch.sa[2] = mine
            c.ledger_reset()
        ch.first(al)
        if what == "unrelated_between":
            c.fill(0.0, other)
        elif what == "second_source_before_its_call":
            c.fill(0.0, mine)  # stored before the pair's launch reads it
        ch.second(al)
        ch.axpys()
        if what == "unrelated_after":
            c.fill(0.0, other)
        dots = ch.dots()
        return ch.finish(dots, [other.numpy(), mine.numpy()])

    got, dl, el, ol = three(sides, run)
    assert pair_launches(dl) == 1
    assert rows(dl)["gemm_outer"] == (2, 8.0 * n * (2 * k + 2 * m)) and calls(dl, "axpy") == 0 and calls(dl, "dot") == 0
    zeroed = got[2 * m + 2] if what == "second_source_before_its_call" else got[2 * m + 1]
    assert zeroed.size == n and not zeroed.any() and not np.signbit(zeroed).any()
    assert calls(dl, "fill") == 1  # the one fill nothing consumed
    check_dots(got[m:2 * m], got[2 * m])


# 4. an infinite element and a -0.0 sum in a destination of the first call, with and without its term
@pytest.mark.parametrize("attach", ["all", "none", "subset"])
def test_infinite_element_and_negative_zero(sides, attach):
    n, m, k = 4099, 3, 1
    al = np.array([[-1e-200, 0.75, -1.25]])
    special = np.random.default_rng(3).uniform(-1, 1, n)
    tiny = [1, 130, 700, 2047, 2048, n - 1]  # window positions of both halves, and the odd last element
    inf = [0, 511, 1029, 4096, 4097]  # and the position past the last whole window
    special[tiny] = 1e-200  # alpha(0, 0) x underflows to -0.0
    special[inf] = [np.inf, -np.inf, np.inf, -np.inf, np.inf]

    def run(s):
        c = s.ctx
        ch = Chain(s, n, m, k, nextra=1)
        c.upload_into(ch.extra[0], special)
        ch.sp[0] = ch.extra[0]
        c.ledger_reset()
        ch.first(al)
        ch.second(al)
        ch.axpys(attach)
        return ch.finish(ch.dots())

    got, dl, el, ol = three(sides, run)
    assert pair_launches(dl) == 1
    check_pair_row(dl, "gemm_outer", n, k, m, nterms(m, attach))
    assert np.all(got[0][tiny] == 0.0) and np.all(np.signbit(got[0][tiny]))  # the -0.0 sums were there
    assert np.all(np.isinf(got[0][inf]))
    for j in range(m):  # the first call's destinations all hold infinities: they reach the second's with a term only
        assert np.isinf(got[2 * m][j]) == ATTACH[attach](j)


# 5. repeated and reordered queries are served; anything that may change a vector forgets the sums
def test_repeated_and_reordered_queries(sides):
    n, m, k = 4099, 4, 5
    al = coef(k, m)
    order = [2, 0, 2, 3, 1, 1, 0]

    def run(s):
        ch = Chain(s, n, m, k)
        ch.first(al)
        ch.second(al)
        ch.axpys()
        return ch.finish([s.ctx.dot(ch.da[j], ch.da[j]) for j in order] +
                         [s.ctx.dot_scaled(ch.da[1], 1.0, ch.da[1], 1.0)])

    got, dl, el, ol = three(sides, run)
    assert pair_launches(dl) == 1
    check_pair_row(dl, "gemm_outer", n, k, m, m)
    assert calls(el, "dot") == len(order) + 1
    check_dots([got[m + j] for j in order + [1]], got[2 * m])


@pytest.mark.parametrize("what", ["axpy", "scal", "upload", "fill", "free_realloc"])
def test_invalidation(sides, what):
    n, m, k = 70001, 3, 5
    al = coef(k, m)
    fresh = host_x(n, 40)

    def run(s):
        c = s.ctx
        ch = Chain(s, n, m, k, nextra=1)
        ch.first(al)
        ch.second(al)
        ch.axpys()
        da = ch.da
        d0 = c.dot(da[0], da[0])
        if what == "axpy":
            c.axpy(0.75, ch.extra[0], da[1])
        elif what == "scal":
            c.scal(-1.5, da[1])
        elif what == "upload":
            c.upload_into(da[1], fresh)
        elif what == "fill":
            c.fill(0.0, da[1])
        else:
            ptr = da[1].ptr
            da[1].free()
            held = []  # the arena hands out its cached blocks of this size oldest first
            for _ in range(512):
                v = c.alloc(n)
                if v.ptr == ptr:
                    break
                held.append(v)
            assert v.ptr == ptr  # the same address and n, new data
            c.upload_into(v, fresh)
            da[1] = v
            for h in held:
                h.free()
        dots = [d0] + [c.dot(v, v) for v in da[1:]]
        return ch.finish(dots)

    got, dl, el, ol = three(sides, run)
    assert pair_launches(dl) == 1
    assert rows(dl)["gemm_outer"] == (2, 8.0 * n * (2 * k + 2 * m))
    assert calls(dl, "dot") == m - 1 and calls(el, "dot") == m  # only the first was served
    check_dots(got[m:2 * m], got[2 * m])
    if what == "fill":
        assert got[2 * m][1] == 0.0
    if what in ("upload", "free_realloc"):
        assert np.array_equal(got[m + 1], fresh)


# 6. SSP_OUTER_PAIR=0: the rows of before the pair for the headline chain
@pytest.mark.parametrize("n,m,k", [(2049, 1, 1), (2248, 3, 5), (4099, 8, 48), (70001, 4, 13)])
def test_switch(sides, n, m, k):
    al = coef(k, m)
    for set_form in (False, True):
        row = "gemm_outer_set" if set_form else "gemm_outer"
        got, dl, el, ol = three(sides, lambda s: run_chain(s, n, m, k, al, "all", set_form))
        assert pair_launches(dl) == 1 and pair_launches(ol) == 0
        # the first call alone, then the second with its m epilogue terms as the norm-carrying instance
        assert rows(ol)[row] == (2, 8.0 * n * (2 * k + 2 * m + m))
        tags = sorted(name for name in ol if name.startswith(row + " [") and ol[name]["calls"])
        assert len(tags) == 2 and sum(f"epi{m} nrm" in t for t in tags) == 1, tags
        assert calls(ol, "axpy") == 0 and calls(ol, "dot") == 0 and calls(ol, "fill") == 0


# 7. two ranks on one device over the host hub: each served dot reduces its own rank-local sum
def test_two_ranks():
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", SSP_HUB_PORT=str(port))
        for name in ENV:
            env.pop(name, None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "outer_pair_worker.py")], env=env,
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
        assert p.returncode == 0 and "outer_pair OK" in out, f"rank {rank} failed:\n{out[-4000:]}"
