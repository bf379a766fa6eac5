#!/usr/bin/env python3
"""Measurements of the refined f32 Q space under a Q-space limit (profiles/r14/q32_refined_dspace.md):

  dense     dense_3000, 3 roots at 1e-10, limit 30: the f64 solve against refined + consistent D space
  synth     synthetic N (default 1e7), 8 roots at 1e-8, Q <= 48 and Q <= 16: the same pair; iterations, actions, wall and
            kernel time (the library's HIP-event ledger), arena bytes after the solve (ssp_memory_stats: in use +
            cached, the cache released before each solve, so this is the solve's footprint)
  combine   ssp_q32_combine_widen at N, 16 -> 8, against ssp_mx_gemm_outer(set) + 8 ssp_mx_copy in the same
            process: median of 10 after 2 warm-ups, variants alternating, each timed by the ledger (kernel time)

Prints markdown.  Usage: q32_dspace.py [--n N] [dense] [synth] [combine]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iterative-solver_amd"))
import itsolv_hbm as ih  # noqa: E402
import subspace_hip as sh  # noqa: E402


def solve_pair(ctx, label, call, kw, limit):
    rows = []
    for name, extra in (("f64", {}), ("refined + dspace", dict(q32=True, refine=True, refine_dspace=True))):
        ctx.synchronize()
        ctx.release_cached()
        ctx.ledger_reset()
        ctx.ledger_enable(True)
        r = call(**dict(kw, max_size_qspace=limit, **extra))
        ctx.synchronize()
        ctx.ledger_enable(False)
        led = ctx.ledger()
        in_use, cached = ctx.memory_stats()
        act = sum(v["calls"] for op, v in led.items() if "action" in op.split("(")[0].split(" [")[0])
        st, ds = r.get("refine", {}), r.get("refine_dspace", {})
        rows.append(f"| {label} | {name} | {r['converged']} | {r['iterations']} | {act} | {st.get('refined_actions', 0)} | "
                    f"{ds.get('dspace_rebuilds', '-')} | {ds.get('dspace_actions', 0)} | {r['seconds']:.3f} | "
                    f"{sum(v['ms'] for v in led.values()) / 1e3:.3f} | {(in_use + cached) / 2**30:.2f} | "
                    f"{np.max(r['errors']):.2e} | {np.max(r['residual_norms']):.2e} |")
    return rows


HEAD = ["| problem | Q space | converged | iterations | action calls | refined actions | rebuilds | D actions | wall s | "
        "kernel s | arena GiB | max error | max residual norm |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]


def dense(ctx):
    n = 3000
    b = np.random.default_rng(7).uniform(-1, 1, (n, n)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(n), np.arange(n)] = 1 + 9 * np.arange(n) / n
    kw = dict(nroots=3, convergence_threshold=1e-10, max_iter=100)
    return solve_pair(ctx, "dense_3000, 1e-10, Q <= 30", lambda **k: ih.davidson_dense(ctx, h, **k), kw, 30)


def synth(ctx, n):
    kw = dict(nroots=8, convergence_threshold=1e-8, max_iter=100, solutions=False)
    call = lambda **k: ih.davidson_synthetic(ctx, n, 0.1, 2, 20251015, **k)  # noqa: E731
    # Q <= 48 is the headline configuration; Q <= 16 is added because the headline solve ends before it reaches 48
    return (solve_pair(ctx, f"synthetic N = {n}, 8 roots, 1e-8, Q <= 48", call, kw, 48) +
            solve_pair(ctx, f"synthetic N = {n}, 8 roots, 1e-8, Q <= 16", call, kw, 16))


def combine(ctx, n, k=16, m=8, reps=10, warm=2):
    r = np.random.default_rng(1)
    xx = [ctx.alloc(n, np.float32) for _ in range(k)]
    for i, x in enumerate(xx):
        ctx.fill(0.5 + 0.01 * i, x)
    al = r.uniform(-1, 1, (k, m))
    y = [ctx.alloc(n, np.float32) for _ in range(m)]
    w = [ctx.alloc(n) for _ in range(m)]

    def two():
        ctx.mx_gemm_outer(al, xx, y, set=True)
        for a, b in zip(w, y):
            ctx.mx_copy(a, b)

    variants = [("gemm_outer(set) + 8 copies", two, (4.0 * k + 4 * m + 12 * m) * n),
                ("combine_widen", lambda: ctx.q32_combine_widen(al, xx, y, w), (4.0 * k + 12 * m) * n)]
    ms = {label: [] for label, _, _ in variants}
    for it in range(warm + reps):
        for label, call, _ in variants:
            ctx.ledger_reset()
            ctx.ledger_enable(True)
            call()
            ctx.synchronize()
            ctx.ledger_enable(False)
            if it >= warm:
                ms[label].append(sum(v["ms"] for v in ctx.ledger().values()))
    out = ["| N | shape | variant | median ms | min | max | GB/s on its own bytes | ratio |", "|---|---|---|---|---|---|---|---|"]
    base = statistics.median(ms[variants[0][0]])
    for label, _, nbytes in variants:
        med = statistics.median(ms[label])
        out.append(f"| {n} | {k} -> {m} | {label} | {med:.3f} | {min(ms[label]):.3f} | {max(ms[label]):.3f} | "
                   f"{nbytes / med / 1e6:.0f} | {med / base:.3f} |")
    for v in xx + y + w:
        v.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("what", nargs="*", default=["dense", "synth", "combine"])
    a = ap.parse_args()
    with sh.Context(0) as ctx:
        rows = []
        if "dense" in a.what:
            rows += dense(ctx)
        if "synth" in a.what:
            rows += synth(ctx, a.n)
        if rows:
            print("\n".join(HEAD + rows), flush=True)
        if "combine" in a.what:
            print()
            print("\n".join(combine(ctx, a.n)), flush=True)


if __name__ == "__main__":
    main()
