#!/usr/bin/env python3
"""In-solver ledger: run whole solves on one MI355X with the per-op HIP-event
ledger enabled and report, per handler operation, calls, kernel time, algorithmic bytes and GB/s,
plus the solve's wall time.  Complements bench.py (a fixed subspace-update step) with the op mix
of real Davidson / DIIS iterations.

usage: python tools/solver_ledger.py [--configs C2,C2-mgs,C3,C3-mgs,C5,C4-shard] [--q32] [--refine] [--no-q-limit]
                                     [--threshold T] [--out profiles/r1/solver_ledger.json]
--refine: the Davidson configs on the refined f32 Q space (include/itsolv_hbm.h *_q32_refined); its scope has no
Q-space limit and no D space, so max_size_qspace and reset_D are dropped from the config.  --no-q-limit drops
them for the other modes too (the like-for-like baselines); --threshold overrides convergence_threshold.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iterative-solver_amd"))

import itsolv_hbm as ih  # noqa: E402
import subspace_hip as sh  # noqa: E402

CONFIGS = {
    # name: (solver, n, kwargs) -- H = diag(1 + i) + rho * sum_l u_l u_l^T (rank 8 for steady state)
    "C2": ("davidson", 10_000_000, dict(rho=0.1, rank=8, seed=1, nroots=4, max_size_qspace=24, reset_D=8,
                                         convergence_threshold=1e-8)),
    "C3": ("davidson", 100_000_000, dict(rho=0.1, rank=8, seed=1, nroots=8, max_p=16, max_size_qspace=48,
                                          reset_D=8, convergence_threshold=1e-8)),
    # the same with the reference's sequential MGS (itsolv_options.block_gram_schmidt = 0; the HBM
    # handlers' default is block Gram-Schmidt)
    "C3-mgs": ("davidson", 100_000_000, dict(rho=0.1, rank=8, seed=1, nroots=8, max_p=16, max_size_qspace=48,
                                              reset_D=8, convergence_threshold=1e-8, block_gram_schmidt=0)),
    "C2-mgs": ("davidson", 10_000_000, dict(rho=0.1, rank=8, seed=1, nroots=4, max_size_qspace=24, reset_D=8,
                                             convergence_threshold=1e-8, block_gram_schmidt=0)),
    # C5's well-posed DIIS instance (itsolv_hbm.c5_spec; tests/golden/traces.json C5_n1e8)
    "C5": ("diis", 100_000_000, dict(**ih.c5_spec(100_000_000), max_size_qspace=6, convergence_threshold=1e-8)),
    # the round-1 instance (chaotic past its 1e-6 plateau)
    "C5x": ("diis", 100_000_000, dict(rho=0.01, rank=3, seed=3, max_size_qspace=6, convergence_threshold=1e-8)),
    # one rank's shard of C4 (N = 1e8 over 8 GPUs): the C3 problem at N = 1.25e7 (run with --rccl for
    # the multi-rank reduction path: fold -> ncclAllReduce -> publish)
    "C4-shard": ("davidson", 12_500_000, dict(rho=0.1, rank=8, seed=1, nroots=8, max_p=16, max_size_qspace=48,
                                              reset_D=8, convergence_threshold=1e-8)),
}
REDUCING = ("dot", "gemm_inner", "axpy_inner", "scal_inner", "axpy_norm", "axpy_gram", "axpy_pairs_norm", "select", "gemm_inner_sparse",
            # a Q space stored in f32 (--q32)
            "dot_f32", "gemm_inner_f32", "gemm_inner_cols")
Q32 = False  # --q32: the Davidson configs with the Q space stored in f32
REFINE = False  # --refine: ... in the refined mode
NO_Q_LIMIT = False  # --no-q-limit
THRESHOLD = None  # --threshold


def run(ctx, name, repeat=2):
    """Solves `repeat` times in one context and reports the last (HBM arena warm); the first
    (cold: every vector block is a fresh hipMalloc) wall time is reported beside it."""
    cold = None
    for _ in range(repeat - 1):
        cold = run_once(ctx, name)["wall_s"]
    out = run_once(ctx, name)
    out["wall_s_cold"] = cold
    print(json.dumps({k: out[k] for k in ("config", "converged", "iterations", "wall_s", "wall_s_cold", "kernel_ms", "kernel_GBs", "reductions_per_iteration", "host_overhead_ms", "host_algebra",
                                            "wall_GBs", "refine") if k in out}), flush=True)
    return out


def run_once(ctx, name):
    solver, n, kw = CONFIGS[name]
    kw = dict(kw)
    rho, rank, seed = kw.pop("rho"), kw.pop("rank"), kw.pop("seed")
    if solver == "davidson" and (REFINE or NO_Q_LIMIT):
        for k in ("max_size_qspace", "reset_D", "reset_D_max_Q_size"):
            kw.pop(k, None)
    if THRESHOLD is not None:
        kw["convergence_threshold"] = THRESHOLD
    ctx.ledger_reset()
    ctx.ledger_enable(True)
    t0 = time.perf_counter()
    if solver == "davidson":
        r = ih.davidson_synthetic(ctx, n, rho, rank, seed, n_local=0, q32=Q32 or REFINE, refine=REFINE, **kw)
    else:
        r = ih.diis_synthetic(ctx, n, rho, rank, seed, n_local=0, **kw)
    wall = time.perf_counter() - t0
    ctx.ledger_enable(False)
    led = ctx.ledger()
    ms = sum(v["ms"] for v in led.values())
    nb = sum(v["bytes"] for v in led.values())
    ops = {op: {"calls": v["calls"], "ms": round(v["ms"], 3), "GB": round(v["bytes"] / 1e9, 3),
                "GBs": round(v["bytes"] / (v["ms"] / 1e3) / 1e9, 1) if v["ms"] > 0 else None,
                "share_of_kernel_time": round(v["ms"] / ms, 4) if ms else None}
           for op, v in sorted(led.items(), key=lambda kv: -kv[1]["ms"])}
    tag = ("-q32-refined" if REFINE else "-q32" if Q32 else "") if solver == "davidson" else ""
    out = {"config": name + tag, "solver": solver, "n": n, "options": kw, "converged": r["converged"],
           "iterations": r["iterations"], "wall_s": round(wall, 3), "kernel_ms": round(ms, 3),
           "algorithmic_GB": round(nb / 1e9, 3), "kernel_GBs": round(nb / (ms / 1e3) / 1e9, 1) if ms else None,
           "wall_GBs": round(nb / wall / 1e9, 1), "ops": ops,
           "reductions_per_iteration": round(sum(v["calls"] for op, v in led.items() if op.split("(")[0] in REDUCING)
                                             / max(1, r["iterations"]), 1),
           "launches_per_iteration": round(sum(v["calls"] for v in led.values()) / max(1, r["iterations"]), 1),
           "host_overhead_ms": round(1e3 * wall - ms, 2),
           "host_algebra": {"ms": round(1e3 * r["host_algebra"]["seconds"], 3), "calls": r["host_algebra"]["calls"],
                            "max_dim": r["host_algebra"]["max_dim"]}}
    if solver == "davidson":
        out["eigenvalues"] = [float(e) for e in r["eigenvalues"]]
        out["errors"] = [float(e) for e in r["errors"]]
        out["residual_norms"] = [float(e) for e in r["residual_norms"]]
    if "refine" in r:
        out["refine"] = r["refine"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C2-mgs,C3,C3-mgs,C5")
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "solver_ledger.json"))
    ap.add_argument("--rccl", action="store_true", help="attach a one-rank RCCL communicator (multi-rank path)")
    ap.add_argument("--p2p", action="store_true", help="attach a one-rank peer-memory communicator (multi-rank path)")
    ap.add_argument("--q32", action="store_true", help="Davidson configs with the Q space stored in f32")
    ap.add_argument("--refine", action="store_true", help="... in the refined mode (drops the configs' Q-space limits)")
    ap.add_argument("--no-q-limit", action="store_true", help="drop max_size_qspace / reset_D from the Davidson configs")
    ap.add_argument("--threshold", type=float, default=None, help="override convergence_threshold")
    a = ap.parse_args()
    global Q32, REFINE, NO_Q_LIMIT, THRESHOLD
    Q32, REFINE, NO_Q_LIMIT, THRESHOLD = a.q32, a.refine, a.no_q_limit, a.threshold
    ctx = sh.Context(0)
    if a.rccl:
        ctx.attach_comm(1, 0, sh.Context.unique_id())
    if a.p2p:
        ctx.attach_p2p(1, 0, sh.Context.p2p_unique_id())
    res = [run(ctx, c) for c in a.configs.split(",")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
