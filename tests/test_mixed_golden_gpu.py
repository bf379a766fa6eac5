"""Bit-level record of the mixed-precision kernels (csrc/kernels_mixed.hip) on their bandwidth paths.

The value tests (test_mixed_gpu.py, test_q32_fused_gpu.py) hold the reductions to a tolerance, so a change
of the summation order inside a kernel passes them.  Here every case's output bytes are hashed and compared
with tests/golden/mixed_digests.json, recorded from the library before the kernels were folded into one tile
kernel and shared launchers: a refactoring of that file must reproduce every bit.

Inputs are integers of a seeded generator divided by 3 (a stable stream; the division makes every sum depend
on its order), f32 vectors their rounded copies.  Both sizes lie above the exact path's 2048 elements and keep
every grid below its per-CU cap, so the digests do not depend on the number of CUs: 4133 = 64 * 64 + 37 (a
short remainder, n mod 4 = 1) and 100003 (several hundred workgroups, n mod 4 = 3).  Default environment: no
SSP_* variable set, one rank.

Run as a script (python tests/test_mixed_golden_gpu.py) the module writes the fixture; that is done on the
commit whose bits are to be kept, never on the code under test.
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "mixed_digests.json")
F32, F64 = np.float32, np.float64
PAIRS = [(F32, F32), (F32, F64), (F64, F32)]  # (dtype of x / xx, dtype of y / yy)
SIZES = [4133, 100_003]
INNER = [(1, 1), (3, 5), (8, 48), (48, 8), (17, 65)]           # (m, k): the last two swap, and split launches
COLS = [(3, 1, 1), (8, 16, 48), (16, 5, 7), (17, 20, 50)]      # (m, n64, n32): padding slots, f32-only tiles, >1 tile
OUTER = [(1, 1), (48, 8), (7, 17), (65, 3)]                    # (k, m)
UPDATES = [(2, 48, 8), (0, 65, 17)]                            # (kp, k, m)
OFFSET = 12_345


def tag(dt):
    return "f32" if dt == F32 else "f64"


class Data:
    """The inputs of one case, from a generator seeded by the case id, and the device vectors made of them."""

    def __init__(self, ctx, case_id, n):
        self.ctx, self.n, self.vs = ctx, n, []
        self.rng = np.random.default_rng(zlib.crc32(case_id.encode()))

    def vec(self, dt):
        a = self.rng.integers(-2**20, 2**20, self.n) / 3.0
        v = self.ctx.upload(a.astype(dt), dt)
        self.vs.append(v)
        return v

    def vecs(self, dt, count):
        return [self.vec(dt) for _ in range(count)]

    def coeff(self, *shape):  # in (-1/3, 1/3)
        return self.rng.integers(-2**20, 2**20, shape) / (3.0 * 2**20)

    def scales(self, count):  # in (0.5, 1.17)
        return 0.5 + self.rng.integers(1, 2**20, count) / (3.0 * 2**19)

    def sparse(self, kp):
        """kp sparse vectors of 5 entries (global indices): the shard's first and last element, the n mod 4
        tail, one index outside the shard."""
        ps = []
        for _ in range(kp):
            idx = [OFFSET, OFFSET + self.n - 1, OFFSET + self.n - 2, OFFSET + self.n + 7,
                   OFFSET + int(self.rng.integers(0, self.n))]
            ps.append({j: float(c) for j, c in zip(idx, self.coeff(len(idx)))})
        return ps

    def free(self):
        for v in self.vs:
            v.free()


def interleaved(n64, n32):
    """Column dtypes with the two kinds interleaved evenly, not sorted (and not f64 first)."""
    k = n64 + n32
    return [F64 if (j + 1) * n64 // k > j * n64 // k else F32 for j in range(k)]


def joined(vs):
    return b"".join(v.numpy().tobytes() for v in vs)


def c_copy(d, tx, ty):
    x, y = d.vec(tx), d.vec(ty)
    d.ctx.mx_copy(x, y, 0.7)
    return joined([x])


def c_axpy(d, tx, ty):
    x, y = d.vec(tx), d.vec(ty)
    d.ctx.mx_axpy(-0.37, x, y)
    return joined([y])


def c_scal(d):
    x = d.vec(F32)
    d.ctx.scal(1.3, x)
    return joined([x])


def c_dot(d, tx, ty):
    x, y = d.vec(tx), d.vec(ty)
    return np.float64(d.ctx.mx_dot(x, y)).tobytes()


def c_inner(d, tx, ty, m, k):
    xx, yy = d.vecs(tx, m), d.vecs(ty, k)
    return d.ctx.mx_gemm_inner(xx, yy, xs=d.scales(m), ys=d.scales(k)).tobytes()


def c_cols(d, m, n64, n32):
    rows, cols = d.vecs(F64, m), [d.vec(dt) for dt in interleaved(n64, n32)]
    return d.ctx.q32_gemm_inner_cols(rows, cols, xs=d.scales(m), ys=d.scales(n64 + n32)).tobytes()


def c_outer(d, tx, ty, k, m, set_):
    xx, yy = d.vecs(tx, k), d.vecs(ty, m)
    d.ctx.mx_gemm_outer(d.coeff(k, m), xx, yy, xs=d.scales(k), set=set_)
    return joined(yy)


def c_block_update(d, kp, k, m):
    xx, yy = d.vecs(F32, k), d.vecs(F64, m)
    d.ctx.q32_block_update(d.coeff(kp, m), d.sparse(kp), d.coeff(k, m), xx, yy, d.scales(m), offset=OFFSET)
    return joined(yy)


def c_construct_solution(d, kp, k, m):
    xx, yy = d.vecs(F32, k), d.vecs(F64, m)
    d.ctx.q32_construct_solution(d.coeff(kp, m), d.sparse(kp), d.coeff(k, m), xx, yy, offset=OFFSET)
    return joined(yy)


def cases():
    """{case id: (n, function of a Data, arguments)}"""
    out = {}
    for n in SIZES:
        out[f"scal-f32-n{n}"] = (n, c_scal, ())
        for tx, ty in PAIRS:
            pair = f"{tag(tx)}-{tag(ty)}"
            for name, f in (("mx_copy", c_copy), ("mx_axpy", c_axpy), ("mx_dot", c_dot)):
                out[f"{name}-{pair}-n{n}"] = (n, f, (tx, ty))
            for m, k in INNER:
                out[f"mx_gemm_inner-{pair}-{m}x{k}-n{n}"] = (n, c_inner, (tx, ty, m, k))
            for k, m in OUTER:
                for set_ in (True, False):
                    out[f"mx_gemm_outer-{pair}-{k}to{m}-{'set' if set_ else 'rmw'}-n{n}"] = (n, c_outer, (tx, ty, k, m, set_))
        for m, n64, n32 in COLS:
            out[f"q32_gemm_inner_cols-{m}x{n64}+{n32}-n{n}"] = (n, c_cols, (m, n64, n32))
        for kp, k, m in UPDATES:
            out[f"q32_block_update-{kp}-{k}to{m}-n{n}"] = (n, c_block_update, (kp, k, m))
            out[f"q32_construct_solution-{kp}-{k}to{m}-n{n}"] = (n, c_construct_solution, (kp, k, m))
    return out


CASES = cases()


def digest(ctx, case_id):
    n, f, args = CASES[case_id]
    d = Data(ctx, case_id, n)
    try:
        return hashlib.sha256(f(d, *args)).hexdigest()
    finally:
        d.free()


@pytest.fixture(scope="module")
def golden():
    if not os.path.exists(FIXTURE):
        pytest.fail(f"{FIXTURE} is missing: record it with this module run as a script")
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", list(CASES))
def test_output_bits_equal_the_record(ctx, golden, case_id):
    assert case_id in golden, f"no digest recorded for {case_id}"
    assert digest(ctx, case_id) == golden[case_id]


def test_the_record_has_no_other_cases(golden):
    assert sorted(golden) == sorted(CASES)


if __name__ == "__main__":
    for p in (os.path.join(os.path.dirname(HERE), "iterative-solver_amd"),):
        if p not in sys.path:
            sys.path.insert(0, p)
    import subspace_hip as sh

    with sh.Context(0) as c:
        rec = {case_id: digest(c, case_id) for case_id in CASES}
    target = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(target, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} digests written to {target}")
