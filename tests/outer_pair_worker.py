"""One rank of the two-rank case of tests/test_outer_pair_gpu.py (RANK, WORLD_SIZE, SSP_HUB_PORT in the
environment; reductions over subspace_hip.HubComm, so both ranks share one device).

Each rank holds its shard of every vector on two contexts attached to the same communicator: one as
created by default, one created with SSP_DEFER_OUTER=0 (eager).  The chain of both solution constructions
(fill + gemm_outer twice, or gemm_outer_set twice, the axpys of the first one's destinations onto the
second one's, one norm per destination of the second) runs on both; the vectors and the rank-summed dots
must be the same bits, the default context with one launch for both calls and no "axpy" or "dot" launch
where the pair's kernel exists (m <= 8).  The dots are also held to the rank sum of the downloaded
shards' norms at n eps |y|^2.
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
    sp = [ctx.upload(full.uniform(-1, 1, N)[off:off + ln]) for _ in range(k)]
    sa = [ctx.upload(full.uniform(-1, 1, N)[off:off + ln]) for _ in range(k)]
    dp = [ctx.upload(full.uniform(1, 2, N)[off:off + ln]) for _ in range(m)]
    da = [ctx.upload(full.uniform(1, 2, N)[off:off + ln]) for _ in range(m)]
    al = np.random.default_rng(1000 * k + m).uniform(-1, 1, (k, m))
    a = -np.random.default_rng(m).uniform(0.5, 2, m)
    ctx.ledger_reset()
    for src, dst in ((sp, dp), (sa, da)):
        if set_form:
            ctx.gemm_outer_set(al, src, dst)
        else:
            for v in dst:
                ctx.fill(0.0, v)
            ctx.gemm_outer(al, src, dst)
    for j in range(m):
        if j % 3 != 1:
            ctx.axpy(a[j], dp[j], da[j])
    dots = np.array([ctx.dot(v, v) for v in da] + [ctx.dot(da[0], da[0])])  # the first one twice
    ledger = ctx.ledger()
    got = [v.numpy() for v in dp + da]
    for v in sp + sa + dp + da:
        v.free()
    return got, dots, ledger


def calls(ledger, op):
    return ledger.get(op, {"calls": 0})["calls"]


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    comm = sh.HubComm(rank, world, "127.0.0.1", int(os.environ["SSP_HUB_PORT"]))
    on = sh.Context(0)
    os.environ["SSP_DEFER_OUTER"] = "0"
    eager = sh.Context(0)
    del os.environ["SSP_DEFER_OUTER"]
    for c in (on, eager):
        c.attach_host_comm(comm)
        c.ledger_enable(True)
    off, ln = sh.shard_range(N, world, rank)
    for m, k, set_form in ((1, 1, False), (3, 5, True), (8, 48, False), (16, 5, False)):
        ga, da, la = chain(on, off, ln, m, k, set_form)
        gb, db, lb = chain(eager, off, ln, m, k, set_form)
        for x, y in zip(ga, gb):
            assert np.array_equal(x, y) and np.array_equal(np.signbit(x), np.signbit(y)), (m, k)
        assert np.array_equal(da, db), (m, k, da, db)
        paired = m <= 8
        e = sum(j % 3 != 1 for j in range(m))
        row = "gemm_outer_set" if set_form else "gemm_outer"
        assert la[row]["calls"] == 2 and la[row]["bytes"] == 8.0 * ln * (2 * k + 2 * m + (0 if paired else e)), (m, la)
        assert calls(la, "axpy") == 0 and calls(la, "dot") == (0 if paired else m + 1), (m, la)
        assert lb[row]["calls"] == 2 and lb[row]["bytes"] == 8.0 * ln * (2 * k + 2 * m)
        assert calls(lb, "axpy") == e and calls(lb, "dot") == m + 1
        ref = comm.allreduce(np.array([float(np.dot(v, v)) for v in ga[m:]]))
        assert np.all(np.abs(da[:m] - ref) <= N * EPS * ref), (da, ref)
        assert da[m] == da[0]
    on.close()
    eager.close()
    comm.barrier()
    comm.close()
    print("outer_pair OK")


if __name__ == "__main__":
    main()
