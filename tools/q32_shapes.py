#!/usr/bin/env python3
"""The headline panel shapes with the Q space stored in f32, against the f64 entry points.

One process, one context, the same R vectors for both variants; the f32 Q vectors hold the f64 ones'
values rounded.  Per shape and size: 5 warm-up launches of each variant, then 20 timed pairs, the two
variants alternating launch by launch, each launch timed by the library's HIP-event ledger (kernel
time on the stream, read after a synchronise).  Reported: the median launch time, the rate on the
variant's OWN algorithmic bytes (4 per f32 element, 8 per f64 element), and the ratio of the medians
beside the byte model's.

    python tools/q32_shapes.py [--out FILE] [--sizes 100000000,12500000]

Shapes: gemm_outer 48 -> 8 read-modify-write, gemm_outer_set 48 -> 8, gemm_inner 8 x 48, and the overlap
rows of a subspace update at the C3 column mix (8 new parameters against 8 + 8 f64 columns and 48 + 48 + 8 + 8
f32 ones): the six overlaps of the call-by-call form against one ssp_q32_gemm_inner_cols (--no-rows skips
it: it holds 112 f32 vectors).
"""
import argparse
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iterative-solver_amd"))
import subspace_hip as sh  # noqa: E402

M, K, WARMUP, TIMED = 8, 48, 5, 20


def timed(ctx, name, call):
    """name: the ledger row of a one-launch variant, or None: every row the variant's calls leave, summed."""
    ctx.ledger_reset()
    ctx.ledger_enable(True)
    call()
    ctx.synchronize()
    led = ctx.ledger()
    ctx.ledger_enable(False)
    if name is None:
        return sum(e["ms"] for e in led.values()), sum(e["bytes"] for e in led.values())
    e = led[name]
    assert e["calls"] == 1, (name, e)
    return e["ms"], e["bytes"]


def measure(ctx, variants):
    """variants: [(label, ledger name, call)] -> {label: (median ms, min ms, max ms, bytes)}"""
    for _ in range(WARMUP):
        for _, _, call in variants:
            call()
    ctx.synchronize()
    ms = {label: [] for label, _, _ in variants}
    nbytes = {}
    for _ in range(TIMED):
        for label, name, call in variants:  # alternating, launch by launch
            t, b = timed(ctx, name, call)
            ms[label].append(t)
            nbytes[label] = b
    return {label: (statistics.median(v), min(v), max(v), nbytes[label]) for label, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="100000000,12500000")
    ap.add_argument("--no-rows", action="store_true", help="skip the overlap-rows shape (112 f32 vectors)")
    args = ap.parse_args()
    if sh.device_count() < 1:
        raise SystemExit("q32_shapes: no HIP device visible (a timing needs the GPU)")
    lines = ["# Q space in f32 against f64: the headline panel shapes", "",
             f"One process, {WARMUP} warm-up and {TIMED} timed launches per variant, alternating; kernel time from the",
             "HIP-event ledger; GB/s on each variant's own algorithmic bytes; ratio = second variant's median / the",
             "first's (f32 Q / f64; for the overlap rows one mixed call / the six calls it replaces).", "",
             "| N | shape | variant | median ms | min | max | GB/s | ratio | byte model |", "|---|---|---|---|---|---|---|---|---|"]
    al = np.array([[1e-3 * ((i * M + j) % 17 - 8) for j in range(M)] for i in range(K)])
    with sh.Context(0) as ctx:
        for n in [int(s) for s in args.sizes.split(",")]:
            r = [ctx.alloc(n) for _ in range(M)]
            q64 = [ctx.alloc(n) for _ in range(K)]
            q32 = [ctx.alloc(n, np.float32) for _ in range(K)]
            for i, v in enumerate(r + q64):
                ctx.fill_random(v, 7, i)
            for a, b in zip(q32, q64):
                ctx.mx_copy(a, b)
            shapes = [
                ("gemm_outer 48->8 rmw", 0.625,
                 [("f64", "gemm_outer", lambda: ctx.gemm_outer(al, q64, r)),
                  ("f32 Q", "gemm_outer_f32", lambda: ctx.mx_gemm_outer(al, q32, r))]),
                ("gemm_outer_set 48->8", (4 * K + 8 * M) / (8 * K + 8 * M),
                 [("f64", "gemm_outer_set", lambda: ctx.gemm_outer_set(al, q64, r)),
                  ("f32 Q", "gemm_outer_f32", lambda: ctx.mx_gemm_outer(al, q32, r, set=True))]),
                ("gemm_inner 8x48", (8 * M + 4 * K) / (8 * M + 8 * K),
                 [("f64", "gemm_inner", lambda: ctx.gemm_inner(r, q64)),
                  ("f32 Q", "gemm_inner_f32", lambda: ctx.mx_gemm_inner(r, q32))]),
            ]
            extra = []
            if not args.no_rows:
                # the overlap rows: f64 columns [params, actions], f32 columns [Q params, Q actions, D params, D actions]
                extra = [ctx.alloc(n, np.float32) for _ in range(112 - K)]
                for a, b in zip(extra, q64 + q64):
                    ctx.mx_copy(a, b)
                act = q64[:M]
                qp, qa, dp, da = q32, extra[:K], extra[K:K + 8], extra[K + 8:K + 16]

                def six_calls():
                    ctx.gemm_inner(r, r)
                    ctx.mx_gemm_inner(r, qp)
                    ctx.mx_gemm_inner(r, dp)
                    ctx.gemm_inner(r, act)
                    ctx.mx_gemm_inner(r, qa)
                    ctx.mx_gemm_inner(r, da)

                cols = r + act + qp + qa + dp + da
                shapes.append(("overlap rows 8 x (16 f64 + 112 f32)", (8 * M + 8 * 16 + 4 * 112) / (6 * 8 * M + 8 * 16 + 4 * 112),
                               [("six calls", None, six_calls),
                                ("one mixed call", "gemm_inner_cols", lambda: ctx.q32_gemm_inner_cols(r, cols))]))
            for shape, model, variants in shapes:
                res = measure(ctx, variants)
                first = variants[0][0]
                for label, (med, lo, hi, nb) in res.items():
                    f32 = label != first
                    ratio = f"{res[label][0] / res[first][0]:.3f}" if f32 else ""
                    lines.append(f"| {n:.3g} | {shape} | {label} | {med:.3f} | {lo:.3f} | {hi:.3f} | "
                                 f"{nb / (med * 1e-3) / 1e9:.0f} | {ratio} | {f'{model:.3f}' if f32 else ''} |")
            for v in r + q64 + q32 + extra:
                v.free()
            ctx.release_cached()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
