"""ssp_q32_combine_widen (include/subspace_hip.h): new f32 vectors as combinations of f32 sources, with their f64
twins, in one write-only pass -- bit for bit, in both outputs, the two-call sequence it replaces:

    ssp_mx_gemm_outer(F32 -> F32, set = 1)    then    ssp_mx_copy(w, SSP_F64, y, SSP_F32, 1.0)

Lengths: 1, 3, 4, 5 (the n mod 4 tail with and without a whole quad), 255, 1027 (one partial window), 2048 and
2049 (either side of the default exact_max), 100003 (many windows, more than one workgroup, an odd tail); and
n = 4099 with exact_max raised to 16384 (the exact path on a length the bandwidth path would take).  Sources:
1, 7, 8, 9 (the batch of 8 loads and its remainder), 65 (one more than a launch's 64: the chained launches, the
last of which writes the twins).  Destinations: 1, 2, 3, 8, 9, 17 (every M instance of the kernel, and one
more than a launch's 16).  Every destination starts from a NaN pattern, so an element left unwritten shows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
EXACT_MAX_DEFAULT = 2048
LENGTHS = [1, 3, 4, 5, 255, 1027, 2048, 2049, 100003]
SHAPES = [(1, 1), (9, 3), (65, 17)]
BIG = 100003


def data(k, m, n, seed):
    r = np.random.default_rng(seed)
    xs = [(r.uniform(-2, 2, n) * 10.0 ** r.integers(-3, 4, n)).astype(F32) for _ in range(k)]
    al = r.uniform(-1, 1, (k, m)) * 10.0 ** r.integers(-2, 3, (k, m))
    return xs, al


class Outputs:
    """m f32 destinations and m f64 twins, every element a NaN pattern of its own set."""

    def __init__(self, ctx, m, n):
        self.y = [ctx.upload(np.full(n, np.nan, dtype=F32), F32) for _ in range(m)]
        self.w = [ctx.upload(np.full(n, np.nan)) for _ in range(m)]

    def bits(self):
        return [v.numpy().view(np.uint32).copy() for v in self.y], [v.numpy().view(np.uint64).copy() for v in self.w]

    def free(self):
        for v in self.y + self.w:
            v.free()


def two_calls(ctx, al, xx, out):
    ctx.mx_gemm_outer(al, xx, out.y, set=True)
    for w, y in zip(out.w, out.y):
        ctx.mx_copy(w, y)


def compare(ctx, k, m, n, seed):
    xs, al = data(k, m, n, seed)
    xx = [ctx.upload(x, F32) for x in xs]
    ref, got = Outputs(ctx, m, n), Outputs(ctx, m, n)
    two_calls(ctx, al, xx, ref)
    ctx.q32_combine_widen(al, xx, got.y, got.w)
    (ry, rw), (gy, gw) = ref.bits(), got.bits()
    for j in range(m):
        assert not np.any(np.isnan(got.y[j].numpy())), (k, m, n, j)
        assert np.array_equal(gy[j], ry[j]), (k, m, n, j, "f32 destination")
        assert np.array_equal(gw[j], rw[j]), (k, m, n, j, "f64 twin")
        assert np.array_equal(got.w[j].numpy(), got.y[j].numpy().astype(F64)), (k, m, n, j, "twin = widened")
    for v in xx:
        v.free()
    ref.free()
    got.free()


@pytest.fixture
def exact_max(ctx, request):
    ctx.set_exact_max(request.param)
    yield request.param
    ctx.set_exact_max(EXACT_MAX_DEFAULT)


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("n", LENGTHS)
def test_both_outputs_are_the_two_call_sequence_bit_for_bit(ctx, n, k, m):
    compare(ctx, k, m, n, seed=n + 7 * k + m)


@pytest.mark.parametrize("k", [1, 7, 8, 9, 65])
def test_every_source_count(ctx, k):
    compare(ctx, k, 3, BIG, seed=100 + k)


@pytest.mark.parametrize("m", [1, 2, 3, 8, 9, 17])
def test_every_destination_count(ctx, m):
    compare(ctx, 9, m, BIG, seed=200 + m)


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("exact_max", [16384], indirect=True)
def test_exact_mode_on_a_length_of_the_bandwidth_path(ctx, exact_max, k, m):
    compare(ctx, k, m, 4099, seed=300 + k)


def test_one_rounding_of_the_f64_sum(ctx):
    """Against exact rational arithmetic on a length of the bandwidth path: each element is the fma chain over
    the sources in order (every fma rounded once to f64), rounded once to f32 at the end -- not the per-axpy
    rounding of an f32 accumulation."""
    from fractions import Fraction

    k, m, n = 5, 2, 4100
    xs, al = data(k, m, n, 11)
    xx = [ctx.upload(x, F32) for x in xs]
    out = Outputs(ctx, m, n)
    ctx.q32_combine_widen(al, xx, out.y, out.w)
    for j in range(m):
        got = out.y[j].numpy()
        for e in np.random.default_rng(j).integers(0, n, 64):
            acc = 0.0
            for i in range(k):  # float(Fraction) rounds to nearest-even: one rounding per fma
                acc = float(Fraction(float(al[i, j])) * Fraction(float(xs[i][e])) + Fraction(acc))
            assert got[e] == np.float32(acc), (j, e)
    for v in xx:
        v.free()
    out.free()


def test_ledger_is_one_row_with_the_pass_bytes(ctx):
    k, m, n = 9, 3, BIG
    xs, al = data(k, m, n, 5)
    xx = [ctx.upload(x, F32) for x in xs]
    out = Outputs(ctx, m, n)
    ctx.ledger_reset()
    ctx.ledger_enable(True)
    ctx.q32_combine_widen(al, xx, out.y, out.w)
    ctx.synchronize()
    led = ctx.ledger()
    ctx.ledger_enable(False)
    assert led["combine_widen_f32"]["calls"] == 1 and led["combine_widen_f32"]["bytes"] == (4.0 * k + 12.0 * m) * n, led
    assert "gemm_outer_f32" not in led and "copy_f32" not in led, led
    for v in xx:
        v.free()
    out.free()


def test_pending_zero_fills_on_a_source_and_on_a_destination(ctx):
    """n = 4099 > exact_max: ctx.fill(0.0, .) of an f64 vector is recorded, not launched (csrc/pending_fill.h).
    A source that lies in such a block reads zeros; a twin that is such a block, and an f32 destination that
    lies in one, keep what the pass wrote, and the rest of the destination's block is zero."""
    n = 4099
    xs, al = data(2, 1, n, 3)
    import subspace_hip as sh

    x0 = ctx.upload(xs[0], F32)
    blk = ctx.upload(np.full(n, 7.0))  # 8 n bytes: its first 4 n as an f32 source
    src = sh.DeviceVector(ctx, n, blk.ptr, owner=False, dtype=F32)
    ctx.upload_into(src, xs[1])
    ctx.fill(0.0, blk)
    ref, got = Outputs(ctx, 1, n), Outputs(ctx, 1, n)
    ctx.q32_combine_widen(al, [x0, src], got.y, got.w)
    zero = ctx.upload(np.zeros(n, dtype=F32), F32)
    two_calls(ctx, al, [x0, zero], ref)
    (ry, rw), (gy, gw) = ref.bits(), got.bits()
    assert np.array_equal(gy[0], ry[0]) and np.array_equal(gw[0], rw[0])
    assert np.array_equal(blk.numpy(), np.zeros(n))
    # destinations under pending fills
    wblk, yblk = ctx.upload(np.full(n, 5.0)), ctx.upload(np.full(n, 5.0))
    ydst = sh.DeviceVector(ctx, n, yblk.ptr, owner=False, dtype=F32)
    ctx.fill(0.0, wblk)
    ctx.fill(0.0, yblk)
    ctx.q32_combine_widen(al, [x0, zero], [ydst], [wblk])
    ctx.synchronize()
    assert np.array_equal(ydst.numpy().view(np.uint32), ry[0]) and np.array_equal(wblk.numpy().view(np.uint64), rw[0])
    tail = yblk.numpy()[(n + 1) // 2:]  # the doubles of the block past the f32 destination
    assert np.array_equal(tail, np.zeros(tail.size))
    for v in (x0, blk, zero, wblk, yblk):
        v.free()
    ref.free()
    got.free()


def test_arguments_and_error_strings(ctx):
    n = 8
    x = ctx.upload(np.arange(1.0, 9.0, dtype=F32), F32)
    y = ctx.upload(np.full(n, np.nan, dtype=F32), F32)
    w = ctx.upload(np.full(n, np.nan))
    f = ctx.lib.ssp_q32_combine_widen
    one = lambda v: (C.c_void_p * 1)(v if isinstance(v, int) else v.ptr)
    al = (C.c_double * 1)(2.0)
    err = lambda: ctx.lib.ssp_last_error()
    # m = 0 and n = 0 return at once; k = 0 is the sum of no sources
    assert f(ctx.handle, al, one(x), 1, one(y), one(w), 0, n) == 0
    assert f(ctx.handle, al, one(x), 1, one(y), one(w), 1, 0) == 0
    assert np.all(np.isnan(y.numpy())) and np.all(np.isnan(w.numpy()))
    assert f(ctx.handle, None, None, 0, one(y), one(w), 1, n) == 0
    assert np.array_equal(y.numpy(), np.zeros(n, dtype=F32)) and np.array_equal(w.numpy(), np.zeros(n))
    assert not np.any(np.signbit(y.numpy())) and not np.any(np.signbit(w.numpy()))
    # the plain call
    ctx.q32_combine_widen([[2.0]], [x], [y], [w])
    assert np.array_equal(y.numpy(), 2 * np.arange(1.0, 9.0, dtype=F32)) and np.array_equal(w.numpy(), 2 * np.arange(1.0, 9.0))
    # refusals: each returns SSP_ERR_INVALID and an error that names the entry point and the reason
    def refused(reason, *args):
        assert f(ctx.handle, *args) == 3
        assert b"ssp_q32_combine_widen" in err() and reason in err(), err()

    refused(b"negative dimension", al, one(x), -1, one(y), one(w), 1, n)
    refused(b"negative dimension", al, one(x), 1, one(y), one(w), -1, n)
    refused(b"null alphas", None, one(x), 1, one(y), one(w), 1, n)
    refused(b"null vector list", al, None, 1, one(y), one(w), 1, n)
    refused(b"null vector list", al, one(x), 1, one(y), None, 1, n)
    refused(b"null vector", al, one(x), 1, one(0), one(w), 1, n)
    refused(b"16-byte aligned", al, one(x.ptr + 4), 1, one(y), one(w), 1, 4)
    refused(b"16-byte aligned", al, one(x), 1, one(y), one(w.ptr + 8), 1, 4)
    refused(b"a destination aliases a source", al, one(x), 1, one(x), one(w), 1, n)
    refused(b"a destination aliases a source", al, one(x), 1, one(y), one(x), 1, n)
    refused(b"same vector", al, one(x), 1, one(y), one(y), 1, n)
    with pytest.raises(TypeError):
        ctx.q32_combine_widen([[1.0]], [w], [y], [w])
    with pytest.raises(ValueError):
        ctx.q32_combine_widen([[1.0]], [x], [y], [])
    # nothing above wrote through a refused call
    assert np.array_equal(y.numpy(), 2 * np.arange(1.0, 9.0, dtype=F32))
    for v in (x, y, w):
        v.free()
