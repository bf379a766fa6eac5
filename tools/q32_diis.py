#!/usr/bin/env python3
"""DIIS over a history stored as f32 differences behind f64 anchors, measured (development tool; needs an MI355X).

1. C5 (itsolv_hbm/problems.h c5_spec) at n = 100003 and thresholds 1e-8, 1e-10 and 1e-12: iterations and final
   residuals (recomputed in numpy from x) of the f64 solve and of the f32-difference solve.
2. The two passes at N = 1e7 and 1e8 against their unfused sequences on the same vectors in the same process:
   ssp_q32_store_differences (m = 2) against ssp_copy, ssp_axpy(-1), ssp_mx_copy and ssp_copy per vector;
   ssp_q32_anchor_combine (m = 2, k = 9 and 19 differences: 10 and 20 stored pairs) against ssp_copy and
   ssp_mx_gemm_outer per panel.  The bytes predict 28/68 and (16 + 4k)/(40 + 4k) of the sequences' times.
3. One step's solver passes over a history of 10 and 20 stored pairs, f32 differences against f64 points, at those N.
4. C5 at those N with max_size_qspace = 10 and 20: wall time per iteration and the history's bytes of the
   f32-difference solve against the f64 DIIS (the history C5 keeps is what its svd pruning leaves: the points are
   in the table).

Timings are the median of `--reps` calls after 2 warm-ups, each a host clock around work that ends in a stream
synchronisation; the variants alternate in one process.

usage: python tools/q32_diis.py [--out profiles/r17/q32_diis.md] [--reps 10] [--big] [--quick]
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

F32 = np.float32


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


def c5_residual(x):
    n = x.size
    g = np.arange(n, dtype=np.float64) * 0.6180339887498949
    d = 1.0 + 2.0 * (g - np.floor(g))
    e = x - 1.0 / np.sqrt(n)
    return float(np.linalg.norm(d * e + np.sum(e) / n))


def threshold_table(ctx, n):
    lines = ["| threshold | run | converged | iterations | reported error | residual recomputed from x | points held |",
             "|---|---|---|---|---|---|---|"]
    for thr in (1e-8, 1e-10, 1e-12):
        for name, q32 in (("f64", False), ("f32 differences", True)):
            r = ih.diis_synthetic(ctx, n, **ih.c5_spec(n), q32=q32, convergence_threshold=thr, max_iter=60)
            lines.append(f"| {thr:g} | {name} | {r['converged']} | {r['iterations']} | {r['errors'][0]:.3e} | "
                         f"{c5_residual(r['x']):.3e} | {int(r['trace']['nq'][-1])} |")
    return lines


def pass_table(ctx, sizes, reps):
    lines = ["| N | pass | fused | unfused sequence | measured ratio | bytes predict | fused TB/s |", "|---|---|---|---|---|---|---|"]
    for n in sizes:
        m = 2
        vv, aa, yy = ([ctx.alloc(n) for _ in range(m)] for _ in range(3))
        dd = [ctx.alloc(n, F32) for _ in range(m)]
        t, ds = ctx.alloc(n), ctx.alloc(n, F32)
        for j in range(m):
            ctx.fill_random(vv[j], 5, j)
            ctx.fill_random(aa[j], 6, j)

        def store_seq():
            for j in range(m):
                ctx.copy(t, vv[j])
                ctx.axpy(-1.0, aa[j], t)
                ctx.mx_copy(ds, t)
                ctx.copy(aa[j], vv[j])

        fused, seq = median_ms(ctx, [lambda: ctx.q32_store_differences(vv, aa, dd), store_seq], reps)
        lines.append(f"| {n:.0e} | store_differences, m = 2 | {fused:.3f} ms | {seq:.3f} ms | {fused / seq:.2f} | {28 / 68:.2f} | "
                     f"{28 * m * n / (fused * 1e-3) / 1e12:.2f} |")
        for k in (9, 19):
            pool = [ctx.alloc(n, F32) for _ in range(m * k)]
            for i, d in enumerate(pool):
                ctx.mx_copy(d, vv[i % m], 1.0 / (i + 1))
            gam = np.linspace(0.1, 0.9, k)
            panels = [pool[j * k:(j + 1) * k] for j in range(m)]

            def combine_seq():
                for j in range(m):
                    ctx.copy(yy[j], aa[j])
                    ctx.mx_gemm_outer(-gam.reshape(k, 1), panels[j], [yy[j]])

            fused, seq = median_ms(ctx, [lambda: ctx.q32_anchor_combine(gam, aa, panels, yy), combine_seq], reps)
            lines.append(f"| {n:.0e} | anchor_combine, m = 2, k = {k} | {fused:.3f} ms | {seq:.3f} ms | {fused / seq:.2f} | "
                         f"{(16 + 4 * k) / (40 + 4 * k):.2f} | {(16 + 4 * k) * m * n / (fused * 1e-3) / 1e12:.2f} |")
            for d in pool:
                d.free()
        for v in vv + aa + yy + dd + [t, ds]:
            v.free()
        ctx.release_cached()
    return lines


def step_table(ctx, sizes, reps):
    """The solver's own passes of one DIIS step over a history of k points, without the problem's residual:
    f32 differences -- store_differences (m = 2), the row of H (r against itself and the k - 1 residual differences,
    one gemm_inner_cols), anchor_combine for add_vector (m = 2) and for end_iteration (m = 1);
    f64 points (NonLinearEquationsDIIS over f64 vectors) -- the rows of S and of H (one gemm_inner of 1 x k each),
    the two constructions of add_vector and the one of end_iteration (gemm_outer_set, k sources each); its copies
    into the history share storage and move nothing."""
    lines = ["| N | stored pairs | f32 differences | f64 points | ratio | f32 history | f64 history |", "|---|---|---|---|---|---|---|"]
    for n in sizes:
        for k in (10, 20):
            x, r, ax, ar, yx, yr = (ctx.alloc(n) for _ in range(6))
            for j, v in enumerate((x, r, ax, ar)):
                ctx.fill_random(v, 7, j)
            dx = [ctx.alloc(n, F32) for _ in range(k - 1)]
            dr = [ctx.alloc(n, F32) for _ in range(k - 1)]
            nx, nr = ctx.alloc(n, F32), ctx.alloc(n, F32)
            for i in range(k - 1):
                ctx.mx_copy(dx[i], x, 1.0 / (i + 2))
                ctx.mx_copy(dr[i], r, 1.0 / (i + 2))
            qx = [ctx.alloc(n) for _ in range(k)]
            qr = [ctx.alloc(n) for _ in range(k)]
            for i in range(k):
                ctx.fill_random(qx[i], 8, i)
                ctx.fill_random(qr[i], 9, i)
            gam = np.linspace(0.1, 0.9, k - 1)
            c = np.full((k, 1), 1.0 / k)

            def step_q32():
                ctx.q32_store_differences([x, r], [ax, ar], [nx, nr])
                ctx.q32_gemm_inner_cols([r], [r] + dr)
                ctx.q32_anchor_combine(gam, [ax, ar], [dx, dr], [yx, yr])
                ctx.q32_anchor_combine(gam, [ax], [dx], [yx])

            def step_f64():
                ctx.gemm_inner([x], qx)
                ctx.gemm_inner([r], qr)
                ctx.gemm_outer_set(c, qx, [yx])
                ctx.gemm_outer_set(c, qr, [yr])
                ctx.gemm_outer_set(c, qx, [yx])

            t32, t64 = median_ms(ctx, [step_q32, step_f64], reps)
            lines.append(f"| {n:.0e} | {k} | {t32:.3f} ms | {t64:.3f} ms | {t32 / t64:.2f} | {((k - 1) * 8 + 16) * n / 2**30:.2f} GiB | "
                         f"{16 * k * n / 2**30:.2f} GiB |")
            for v in [x, r, ax, ar, yx, yr, nx, nr] + dx + dr + qx + qr:
                v.free()
            ctx.release_cached()
    return lines


def solve_table(ctx, sizes):
    lines = ["| N | max_size_qspace | run | converged | iterations | points held | wall per iteration | kernel time per iteration | "
             "history bytes |", "|---|---|---|---|---|---|---|---|---|"]
    for n in sizes:
        for limit in (10, 20):
            for name, q32 in (("f64", False), ("f32 differences", True)):
                ctx.release_cached()
                ctx.ledger_reset()
                ctx.ledger_enable(True)
                t0 = time.perf_counter()
                r = ih.diis_synthetic(ctx, n, **ih.c5_spec(n), q32=q32, solutions=False, convergence_threshold=1e-8,
                                      max_iter=60, max_size_qspace=limit)
                ctx.synchronize()
                wall = time.perf_counter() - t0
                ctx.ledger_enable(False)
                kernel_ms = sum(v["ms"] for v in ctx.ledger().values())
                k = int(r["trace"]["nq"][-1])
                held = r["diis_q32"]["history_bytes"] if q32 else 16 * k * n
                its = max(1, r["iterations"])
                lines.append(f"| {n:.0e} | {limit} | {name} | {r['converged']} | {r['iterations']} | {k} | {1e3 * wall / its:.2f} ms | "
                             f"{kernel_ms / its:.2f} ms | {held / 2**30:.3f} GiB |")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "q32_diis.md"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--big", action="store_true", help="also solve at N = 1e8")
    ap.add_argument("--quick", action="store_true", help="N = 1e6 only (a smoke run of the tool)")
    args = ap.parse_args()
    psizes = [10**6] if args.quick else [10**7, 10**8]
    ssizes = [10**6] if args.quick else [10**7] + ([10**8] if args.big else [])
    with sh.Context(0) as ctx:
        tlines = threshold_table(ctx, 100_003)
        plines = pass_table(ctx, psizes, args.reps)
        klines = step_table(ctx, psizes, args.reps)
        slines = solve_table(ctx, ssizes)
    text = ["# DIIS over f32 differences behind f64 anchors (tools/q32_diis.py)", "",
            "One MI355X, one process; medians of %d calls after 2 warm-ups, the variants alternating." % args.reps, "",
            "## C5 at n = 100003: the f64 solve and the f32-difference solve below 1e-8", ""] + tlines + ["",
            "## The two passes against their unfused sequences", ""] + plines + ["",
            "## One step's solver passes over a history of 10 and 20 stored pairs", "",
            "The passes the solver itself issues per iteration (the new point taken in, the new row of the DIIS matrix, "
            "the constructions of add_vector and end_iteration), on a history of that many points, without the "
            "problem's residual and preconditioner; history: what that many points hold.", ""] + klines + ["",
            "## C5 under a history limit: time per iteration and the history's bytes", "",
            "Single solves, not medians.  C5's svd pruning keeps 4 points whatever the limit.", "",
            "History bytes: the arena's own count for the f32-difference solve (anchors and differences), 16 N per point "
            "for the f64 solve.  Wall time includes the problem's residual evaluations.", ""] + slines + [""]
    if not args.big and not args.quick:
        text += ["N = 1e8 solves: not measured.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    print("\n".join(text))


if __name__ == "__main__":
    main()
