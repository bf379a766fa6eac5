#!/usr/bin/env python3
"""Linear equations over the f32 Q space, measured (development tool; needs an MI355X).

1. ssp_mx_rhs_residual_norms at N = 1e7 and 1e8, m = 8, right-hand sides stored as f32 and as f64, against the
   sequence it replaces on the same vectors in the same process: ssp_mx_axpy(-1, b, y), ssp_scal(s, y) and
   ssp_dot(y, y) per vector.  The bytes predict 20/44 (f32) and 24/48 (f64) of the sequence's time.
2. The synthetic problem at N = 1e7 (and 1e8 with --big), 8 right-hand sides: the f64 solve at 1e-8, the plain
   q32 solve at 1e-6 and the refined q32 solve at 1e-8 -- iterations, stored Q vectors, refined actions, wall and
   kernel time, bytes the Q space holds, reported errors against recomputed residuals.

Timings are the median of `--reps` calls after 2 warm-ups, each a host clock around work that ends in a stream
synchronisation; the variants alternate in one process.

usage: python tools/q32_lineq.py [--out profiles/r15/q32_lineq.md] [--reps 10] [--big] [--quick]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iterative-solver_amd"))

import itsolv_hbm as ih  # noqa: E402
import subspace_hip as sh  # noqa: E402

M = 8
SYNTH = dict(rho=0.1, rank=4, seed=20251015, nrhs=8, rhs_seed=11)


def median_ms(ctx, fns, reps, warm=2):
    """Median wall time (ms) of each callable, the callables alternating inside every repetition."""
    samples = [[] for _ in fns]
    for rep in range(warm + reps):
        for i, fn in enumerate(fns):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if rep >= warm:
                samples[i].append(1e3 * (time.perf_counter() - t0))
    return [statistics.median(s) for s in samples]


def kernel_table(ctx, sizes, reps):
    lines = ["| N | rhs stored as | fused pass | axpy + scal + dot x m | measured ratio | bytes predict | fused TB/s |",
             "|---|---|---|---|---|---|---|"]
    ratios = {}
    for n in sizes:
        yy = [ctx.alloc(n) for _ in range(M)]
        b64 = [ctx.alloc(n) for _ in range(M)]
        for j in range(M):
            ctx.fill_random(yy[j], 5, j)
            ctx.fill_random(b64[j], 6, j)
        b32 = [ctx.alloc(n, np.float32) for _ in range(M)]
        for j in range(M):
            ctx.mx_copy(b32[j], b64[j])
        s = [1.0 + 2.0**-20] * M  # (the values drift by a rounding per call: no overflow in a few dozen calls)

        def sequence(bb):
            for j in range(M):
                ctx.mx_axpy(-1.0, bb[j], yy[j])
                ctx.scal(s[j], yy[j])
            return [ctx.dot(v, v) for v in yy]

        for name, bb, eb in (("f32", b32, 4), ("f64", b64, 8)):
            fused, seq = median_ms(ctx, [lambda: ctx.mx_rhs_residual_norms(bb, s, yy), lambda: sequence(bb)], reps)
            tbs = n * M * (16 + eb) / (fused * 1e-3) / 1e12
            ratios[(n, name)] = fused / seq
            lines.append(f"| {n:.0e} | {name} | {fused:.3f} ms | {seq:.3f} ms | {fused / seq:.2f} | "
                         f"{(16 + eb) / (40 + eb):.2f} | {tbs:.2f} |")
        for v in yy + b64 + b32:
            v.free()
        ctx.release_cached()
    return lines, ratios


def solve_table(ctx, sizes):
    lines = ["| N | run | threshold | converged | iterations | stored Q vectors | refined actions | wall | kernel time | "
             "Q-space bytes | max reported error | max recomputed residual | max abs(error - residual) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in sizes:
        for name, thr, extra, qbytes in (("f64", 1e-8, {}, 8), ("plain q32", 1e-6, dict(q32=True), 4),
                                         ("refined q32", 1e-8, dict(q32=True, refine=True), 4)):
            ctx.release_cached()
            ctx.ledger_reset()
            ctx.ledger_enable(True)
            t0 = time.perf_counter()
            r = ih.linear_equations_synth(ctx, n, SYNTH["rho"], SYNTH["rank"], SYNTH["seed"], SYNTH["nrhs"],
                                          SYNTH["rhs_seed"], solutions=False, convergence_threshold=thr, **extra)
            ctx.synchronize()
            wall = time.perf_counter() - t0
            ctx.ledger_enable(False)
            kernel_ms = sum(v["ms"] for v in ctx.ledger().values())
            stored = r["q_creations"]  # parameter and action vectors copied into the Q space
            refined = r["refine"]["refined_actions"] if "refine" in r else 0
            held = stored * n * qbytes + (SYNTH["nrhs"] * n * (qbytes + (8 if "refine" in r else 0)))
            lines.append(f"| {n:.0e} | {name} | {thr:g} | {r['converged']} | {r['iterations']} | {stored} | {refined} | "
                         f"{wall:.3f} s | {kernel_ms / 1e3:.3f} s | {held / 2**30:.2f} GiB | {np.max(r['errors']):.3e} | "
                         f"{np.max(r['residual_norms']):.3e} | {np.max(np.abs(r['errors'] - r['residual_norms'])):.3e} |")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "q32_lineq.md"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--big", action="store_true", help="also solve at N = 1e8")
    ap.add_argument("--quick", action="store_true", help="N = 1e6 only (a smoke run of the tool)")
    args = ap.parse_args()
    ksizes = [10**6] if args.quick else [10**7, 10**8]
    ssizes = [10**6] if args.quick else [10**7] + ([10**8] if args.big else [])
    with sh.Context(0) as ctx:
        klines, ratios = kernel_table(ctx, ksizes, args.reps)
        slines = solve_table(ctx, ssizes)
    text = ["# Linear equations over the f32 Q space (tools/q32_lineq.py)", "",
            "One MI355X, one process; medians of %d calls after 2 warm-ups, the variants alternating." % args.reps, "",
            "## ssp_mx_rhs_residual_norms against the sequence it replaces, m = %d" % M, ""] + klines + [""]
    at = min(ksizes)
    slower = [k for k, v in ratios.items() if k[0] == at and v >= 1.0]
    text += ["The fused pass is %s the sequence at N = %.0e%s." % (
        "not faster than" if slower else "faster than", at,
        " for " + ", ".join(k[1] for k in slower) + " right-hand sides" if slower else ""), "",
        "## The synthetic solves, %d right-hand sides (rho = %g, rank %d)" % (SYNTH["nrhs"], SYNTH["rho"], SYNTH["rank"]), "",
        "Q-space bytes: stored Q vectors and right-hand sides at their element size (the refined mode's f64 twins "
        "included); errors and residuals are relative to |b|.", ""] + slines + [""]
    if not args.big and not args.quick:
        text += ["N = 1e8: not measured.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    print("\n".join(text))


if __name__ == "__main__":
    main()
