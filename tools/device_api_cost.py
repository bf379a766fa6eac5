#!/usr/bin/env python3
"""Cost of the device forms of the reverse-communication API (development tool; needs an MI355X).

1. ssp_rows_import / ssp_rows_export at N = 1e7 and 1e8 with m = 8 and 16 rows, aligned rows and rows at
   8 mod 16, against ssp_copy on the same vectors in the same process (ssp_copy is the yardstick).
2. One Davidson solve of the C3 problem at N = 1e7 (8 roots; without the P space, which only the C++ runner
   can enter without a host callback) through the reverse-communication loop with host arrays, with device
   rows, and through itsolv_davidson_synth, the HBM-resident floor.

Everything runs in one process; every figure is the median of `--reps` samples after discarded warm-ups, each
sample a host clock around work that ends in a stream synchronisation.

With --options (repeatable, `OPTIONS[@THRESHOLD]`, "" for none) the tool measures the f32 Q space behind the API
instead: ssp_rows_export_quantised beside the scaled ssp_rows_export, and the device-route solve once per option
set -- wall per iteration, iterations, refined actions, ssp_memory_stats bytes in use at the end.  An option set
with Q_REFINE gets the synthetic action as its refine action and runs without the C3 Q-space limit (the refined
mode has no D space).

usage: python tools/device_api_cost.py [--out profiles/r11/device_api.md] [--reps 11] [--quick]
       python tools/device_api_cost.py --options "" --options Q_STORAGE=f32@1e-6 --options Q_STORAGE=f32,Q_REFINE=1@1e-8
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iterative-solver_amd"))

import iterative_solver  # noqa: E402
import itsolv_hbm as ih  # noqa: E402
import subspace_hip as sh  # noqa: E402

C3 = dict(rho=0.1, rank=8, seed=1, nroots=8, max_size_qspace=48, reset_D=8, convergence_threshold=1e-8)
BIG = 1.7976931348623157e308


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


def rows_table(ctx, sizes, reps):
    lines = ["| N | m | layout | ssp_copy x m | rows_import | rows_export | rows_export, scaled | import / copy |",
             "|---|---|---|---|---|---|---|---|"]
    ratios = []
    for n in sizes:
        for m in (8, 16):
            vecs = [ctx.alloc(n) for _ in range(m)]
            buf = ctx.alloc(m * n + 2)
            for k, v in enumerate(vecs):
                ctx.fill_random(v, 3, k)
            ctx.fill(0.5, buf)
            for layout, base in (("aligned", 0), ("8 mod 16", 1)):
                rows = sh.DeviceRows(ctx, m, n, n, ptr=buf.ptr + 8 * base)
                aligned = [sh.DeviceVector(ctx, n, buf.ptr + 8 * k * n, owner=False) for k in range(m)]
                xs = [0.75] * m

                def copies():
                    for v, r in zip(vecs, aligned):  # the yardstick always moves the aligned rows
                        ctx.copy(v, r)

                t = median_ms(ctx, [copies, lambda: ctx.rows_import(rows, vecs), lambda: ctx.rows_export(vecs, rows),
                                    lambda: ctx.rows_export(vecs, rows, xs)], reps)
                tb = [16.0 * m * n / (1e9 * x) for x in t]  # TB/s: bytes / (ms * 1e9)
                lines.append(f"| {n:.0e} | {m} | {layout} | {t[0]:.3f} ms, {tb[0]:.2f} TB/s | {t[1]:.3f} ms, {tb[1]:.2f} TB/s | "
                             f"{t[2]:.3f} ms, {tb[2]:.2f} TB/s | {t[3]:.3f} ms, {tb[3]:.2f} TB/s | {t[1] / t[0]:.3f} |")
                print(lines[-1], flush=True)
                if base == 0:
                    t_aligned = t
                else:
                    ratios.append(f"N = {n:.0e}, m = {m}: import {t[1] / t_aligned[1]:.2f}, export {t[2] / t_aligned[2]:.2f}")
            for v in vecs + [buf]:
                v.free()
            ctx.release_cached()
    lines += ["", "Time of the misaligned form over the aligned form: " + "; ".join(ratios) + ".  The misaligned rows move with "
              "8-byte accesses on both sides (twice the memory instructions per byte).  The import's misaligned side is its "
              "loads, the export's its stores, whose 512-byte runs then begin 8 bytes off a 128-byte line; that this is why "
              "the export loses more is a supposition, the cause has not been profiled."]
    return lines


def rows_q_table(ctx, sizes, reps):
    """ssp_rows_export_quantised with mq = m beside ssp_rows_export scaled, aligned rows, same process."""
    lines = ["| N | m | rows_export, scaled | rows_export_q, mq = m | q / plain |", "|---|---|---|---|---|"]
    for n in sizes:
        for m in (8, 16):
            vecs = [ctx.alloc(n) for _ in range(m)]
            buf = ctx.alloc(m * n)
            for k, v in enumerate(vecs):
                ctx.fill_random(v, 3, k)
            rows = sh.DeviceRows(ctx, m, n, n, ptr=buf.ptr)
            xs = [0.75] * m
            t = median_ms(ctx, [lambda: ctx.rows_export(vecs, rows, xs), lambda: ctx.rows_export_quantised(vecs, rows, xs, m)],
                          reps)
            tb = [16.0 * m * n / (1e9 * x) for x in t]
            lines.append(f"| {n:.0e} | {m} | {t[0]:.3f} ms, {tb[0]:.2f} TB/s | {t[1]:.3f} ms, {tb[1]:.2f} TB/s | {t[1] / t[0]:.3f} |")
            print(lines[-1], flush=True)
            for v in vecs + [buf]:
                v.free()
            ctx.release_cached()
    return lines


def api_solve(ctx, n, device, max_iter, options=None, thresh=None):
    """One Davidson solve through the reverse-communication loop; returns per-phase wall times.  options: an
    option set of --options (None: the C3 options of the r11 report)."""
    nroot = C3["nroots"]
    limits = f"MAX_SIZE_QSPACE={C3['max_size_qspace']},RESET_D={C3['reset_D']}"
    refines = options is not None and "Q_REFINE=1" in options.upper().replace(" ", "")
    full = limits if options is None else options if refines else ",".join(x for x in (limits, options) if x)
    s = iterative_solver.LinearEigensystem(n, nroot, thresh=thresh or C3["convergence_threshold"], thresh_value=BIG,
                                           hermitian=True, options=full)
    if refines:  # device rows in, device rows out
        s.set_refine_action(lambda x, a: ctx.synthetic_action(x.rows(), a.rows(), C3["rho"], C3["rank"], C3["seed"]))
    px, pg = sh.DeviceRows(ctx, nroot, n), sh.DeviceRows(ctx, nroot, n)
    diag = ctx.alloc(n)
    ctx.synthetic_diagonal(diag, C3["rho"], C3["rank"])
    if options is not None:  # the diagonals as the instance keeps them: in Q storage (rounded for an f32 Q space)
        iterative_solver._dcall("IterativeSolverHbmSetDiagonalsDevice", diag.ptr)
        iterative_solver._dcall("IterativeSolverHbmDiagonalsDevice", diag.ptr)
    if device:
        x, g = px, pg
        for k in range(nroot):
            ctx.sparse_copy(px.row(k), [k], [1.0])
    else:
        x, g = np.zeros((nroot, n)), np.zeros((nroot, n))
        x[np.arange(nroot), np.arange(nroot)] = 1.0
    t_api = t_action = 0.0
    nwork, iters = nroot, 0
    ctx.synchronize()
    ctx.ledger_enable(True)
    ctx.ledger_reset()
    t_start = time.perf_counter()
    for _ in range(max_iter):
        t0 = time.perf_counter()
        if not device:
            px.head(nwork).upload(x[:nwork])
        ctx.synthetic_action(px.rows()[:nwork], pg.rows()[:nwork], C3["rho"], C3["rank"], C3["seed"])
        if not device:
            g[:nwork] = pg.head(nwork).numpy()
        ctx.synchronize()
        t1 = time.perf_counter()
        nwork = s.add_vector(x.head(nwork), g.head(nwork)) if device else s.add_vector(x[:nwork], g[:nwork])
        ctx.synchronize()
        t2 = time.perf_counter()
        t_action += t1 - t0
        t_api += t2 - t1
        iters += 1
        if nwork == 0:
            break
        ev = s.working_set_eigenvalues(nwork)
        t0 = time.perf_counter()
        if not device:
            pg.head(nwork).upload(g[:nwork])
        ctx.precondition(pg.rows()[:nwork], diag, ev)
        if not device:
            g[:nwork] = pg.head(nwork).numpy()
        ctx.synchronize()
        t1 = time.perf_counter()
        nwork = s.end_iteration(x, g)
        ctx.synchronize()
        t2 = time.perf_counter()
        t_action += t1 - t0
        t_api += t2 - t1
        if nwork == 0:
            break
    wall = time.perf_counter() - t_start
    led = ctx.ledger()
    ctx.ledger_enable(False)
    rows_ms = sum(led[k]["ms"] for k in ("rows_import", "rows_export") if k in led)
    rows_ms += sum(v["ms"] for k, v in led.items() if k.startswith("rows_export_q"))
    out = dict(iterations=iters, wall=wall, api=t_api, action=t_action, rows_ms=rows_ms, errors=float(np.max(s.errors)),
               eigenvalue=float(s.eigenvalues[0]), refined_actions=s.refine_statistics()["refined_actions"],
               bytes_in_use=ctx.memory_stats()[0], q_storage=s.q_storage)
    s.finalize()
    for v in (px, pg, diag):
        v.free()
    return out


def solve_table(ctx, n, reps, max_iter):
    iterative_solver.use_context(ctx)
    runs = {"host calls": [], "device calls": [], "itsolv_davidson_synth": []}
    for rep in range(1 + reps):  # the first of each is a warm-up
        for name in runs:
            if name == "itsolv_davidson_synth":
                ctx.synchronize()
                t0 = time.perf_counter()
                r = ih.davidson_synthetic(ctx, n, C3["rho"], C3["rank"], C3["seed"], solutions=False, nroots=C3["nroots"],
                                          max_p=0, max_size_qspace=C3["max_size_qspace"], reset_D=C3["reset_D"],
                                          convergence_threshold=C3["convergence_threshold"])
                ctx.synchronize()
                rec = dict(iterations=r["iterations"], wall=time.perf_counter() - t0, api=float("nan"), action=float("nan"),
                           rows_ms=0.0, errors=float("nan"), eigenvalue=float(r["eigenvalues"][0]))
            else:
                rec = api_solve(ctx, n, name == "device calls", max_iter)
            if rep > 0:
                runs[name].append(rec)
            print(name, rec, flush=True)
    iterative_solver.use_context(None)
    lines = ["| route | iterations | wall per iteration | inside the API calls, per iteration | action + preconditioner, per iteration | "
             "rows_* kernel time, share of wall | lowest eigenvalue |", "|---|---|---|---|---|---|---|"]
    for name, recs in runs.items():
        med = lambda key: statistics.median(r[key] / r["iterations"] for r in recs)  # noqa: E731
        share = statistics.median(1e-3 * r["rows_ms"] / r["wall"] for r in recs)
        lines.append(f"| {name} | {recs[0]['iterations']} | {1e3 * med('wall'):.1f} ms | {1e3 * med('api'):.1f} ms | "
                     f"{1e3 * med('action'):.1f} ms | {100 * share:.1f} % | {recs[0]['eigenvalue']:.12f} |")
    return lines


def options_table(ctx, n, reps, max_iter, option_sets):
    """The device-route solve once per option set of --options."""
    iterative_solver.use_context(ctx)
    runs = {o: [] for o in option_sets}
    for rep in range(1 + reps):  # the first of each is a warm-up
        for o in option_sets:
            opts, _, thresh = o.partition("@")
            rec = api_solve(ctx, n, True, max_iter, opts, float(thresh) if thresh else None)
            if rep > 0:
                runs[o].append(rec)
            print(o or "(none)", rec, flush=True)
    iterative_solver.use_context(None)
    lines = ["| options @ threshold | Q bytes per element | iterations | wall per iteration | inside the API calls, per iteration | "
             "refined actions | largest error at the end | bytes in use at the end | lowest eigenvalue |",
             "|---|---|---|---|---|---|---|---|---|"]
    for o, recs in runs.items():
        med = lambda key: statistics.median(r[key] / r["iterations"] for r in recs)  # noqa: E731
        r0 = recs[0]
        lines.append(f"| `{o or '(none)'}` | {r0['q_storage']} | {r0['iterations']} | {1e3 * med('wall'):.1f} ms | "
                     f"{1e3 * med('api'):.1f} ms | {r0['refined_actions']} | {r0['errors']:.2e} | {r0['bytes_in_use']} | "
                     f"{r0['eigenvalue']:.12f} |")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--options", action="append", default=None, metavar="OPTIONS[@THRESHOLD]",
                    help="measure the f32 Q space behind the API: one device-route solve per option set (repeatable)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "device_api.md"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=40)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    if sh.device_count() < 1:
        raise SystemExit("device_api_cost.py: no HIP device visible")
    ctx = sh.Context(0)
    sizes = (10**5,) if a.quick else (10**7, 10**8)
    n_solve = 10**5 if a.quick else 10**7
    if a.options is not None:
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "r12", "rc_q32_tables.md")
        doc = ["# The f32 Q space behind the reverse-communication API: measured", "",
               f"`tools/device_api_cost.py --reps {a.reps} --solve-reps {a.solve_reps} " +
               " ".join(f'--options "{o}"' for o in a.options) + "`" + (" --quick (REHEARSAL SIZES)" if a.quick else "") +
               ", one process on one MI355X; medians after discarded warm-ups.", "",
               "## ssp_rows_export_quantised beside ssp_rows_export", "", "Bytes are 16 m N, aligned rows, scale 0.75.", ""]
        doc += rows_q_table(ctx, sizes, a.reps)
        doc += ["", f"## Device-route solve, C3 at N = {n_solve:.0e} (8 roots, rank-8 problem, no P space)", "",
                f"Median of {a.solve_reps} solves after one warm-up solve each.  Option sets without Q_REFINE run with the C3 "
                f"limits MAX_SIZE_QSPACE={C3['max_size_qspace']},RESET_D={C3['reset_D']}; one with Q_REFINE runs without "
                "them (the refined mode has no D space).", ""]
        doc += options_table(ctx, n_solve, a.solve_reps, a.max_iter, a.options)
        ctx.close()
        text = "\n".join(doc) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        print(text)
        return
    doc = ["# Device forms of the reverse-communication API: measured cost", "",
           f"`tools/device_api_cost.py --reps {a.reps} --solve-reps {a.solve_reps}`" + (" --quick (REHEARSAL SIZES)" if a.quick else "") +
           ", one process on one MI355X.  Medians of the samples after discarded warm-ups; every sample is a host "
           "clock around work that ends in a stream synchronisation.", "",
           "## ssp_rows_import / ssp_rows_export against ssp_copy", "",
           "Bytes are 16 m N.  `ssp_copy x m` moves the same rows (always the 16-byte aligned ones) with m calls; "
           "`8 mod 16`: the block starts one element into its allocation, so every row is misaligned and moves with "
           "8-byte accesses.", ""]
    doc += rows_table(ctx, sizes, a.reps)
    doc += ["", f"## One Davidson solve, C3 at N = {n_solve:.0e} (8 roots, rank-8 problem, no P space)", "",
            "The same loop three ways: the reverse-communication calls on host arrays (the action and the preconditioner "
            "run on the GPU, so their operands cross PCIe too: the `action` column), the same calls on device rows, and "
            f"the C++ runner.  Median of {a.solve_reps} solves after one warm-up solve each.", ""]
    doc += solve_table(ctx, n_solve, a.solve_reps, a.max_iter)
    ctx.close()
    text = "\n".join(doc) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
