"""One rank of the two-rank case of tests/test_outer_norms_gpu.py (RANK, WORLD_SIZE, SSP_HUB_PORT in the
environment; reductions over subspace_hip.HubComm, so both ranks share one device).

Each rank holds its shard of every vector on two contexts attached to the same communicator: one as
created by default, one created with SSP_OUTER_NORMS=0.  The chain fill + gemm_outer + axpys + one
norm per destination runs on both; the vectors and the rank-summed dots must be the same bits, the
default context with no "dot" launch where the norm-carrying instance exists (m <= 8).  The dots are
also held to the rank sum of the downloaded shards' norms at n eps |y|^2.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "iterative-solver_amd"), HERE):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import subspace_hip as sh  # noqa: E402

EPS = np.finfo(np.float64).eps
N = 140_003  # shards of 70002 and 70001 elements: an even one and one with the odd last element


def chain(ctx, off, ln, m, k, set_form):
    full = np.random.default_rng(5)
    src = [ctx.upload(full.uniform(-1, 1, N)[off:off + ln]) for _ in range(k)]
    own = [ctx.upload(full.uniform(-1, 1, N)[off:off + ln]) for _ in range(m)]
    dst = [ctx.upload(full.uniform(1, 2, N)[off:off + ln]) for _ in range(m)]
    al = np.random.default_rng(1000 * k + m).uniform(-1, 1, (k, m))
    a = -np.random.default_rng(m).uniform(0.5, 2, m)
    ctx.ledger_reset()
    if set_form:
        ctx.gemm_outer_set(al, src, dst)
    else:
        for v in dst:
            ctx.fill(0.0, v)
        ctx.gemm_outer(al, src, dst)
    for j in range(m):
        if j % 3 != 1:
            ctx.axpy(a[j], own[j], dst[j])
    dots = np.array([ctx.dot(v, v) for v in dst] + [ctx.dot(dst[0], dst[0])])  # the first one twice
    ledger = ctx.ledger()
    got = [v.numpy() for v in dst]
    for v in src + own + dst:
        v.free()
    return got, dots, ledger


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    comm = sh.HubComm(rank, world, "127.0.0.1", int(os.environ["SSP_HUB_PORT"]))
    on = sh.Context(0)
    os.environ["SSP_OUTER_NORMS"] = "0"
    off_ctx = sh.Context(0)
    del os.environ["SSP_OUTER_NORMS"]
    for c in (on, off_ctx):
        c.attach_host_comm(comm)
        c.ledger_enable(True)
    off, ln = sh.shard_range(N, world, rank)
    for m, k, set_form in ((1, 1, False), (3, 5, True), (8, 48, False), (16, 5, False)):
        ga, da, la = chain(on, off, ln, m, k, set_form)
        gb, db, lb = chain(off_ctx, off, ln, m, k, set_form)
        for x, y in zip(ga, gb):
            assert np.array_equal(x, y), (m, k)
        assert np.array_equal(da, db), (m, k, da, db)
        served = m <= 8
        assert la.get("dot", {"calls": 0})["calls"] == (0 if served else m + 1), (m, la)
        assert lb["dot"]["calls"] == m + 1
        row = "gemm_outer_set" if set_form else "gemm_outer"
        e = sum(j % 3 != 1 for j in range(m))
        for ledger in (la, lb):
            assert ledger[row]["calls"] == 1 and ledger[row]["bytes"] == 8.0 * ln * (k + m + e)
        ref = comm.allreduce(np.array([float(np.dot(v, v)) for v in ga]))
        assert np.all(np.abs(da[:m] - ref) <= N * EPS * ref), (da, ref)
        assert da[m] == da[0]
    on.close()
    off_ctx.close()
    comm.barrier()
    comm.close()
    print("outer_norms OK")


if __name__ == "__main__":
    main()
