"""The refined mode under a Q-space limit on the CPU (no device): tests/cpp/q32_refined_dspace_model.cpp
instantiates LinearEigensystemDavidson<R, Q, P> with R over double storage and Q over float storage, as
tests/cpp/q32_refined_model.cpp does, and solves the dense_3000 matrix of tests/test_mixed_gpu.py at 1e-10 with
max_size_qspace = LIMIT: with the Q space in f64, and in f32 with set_refine + set_refine_dspace.

What this exercises: the coefficients and the one pass of construct_dspace_refined (through this program's own
fused_new_combinations_widened), the true D actions, the D blocks of update_dspace_refined (call by call), the
refined rows of new_qspace_data with nD != 0, the D terms of the bound, the counters, and the refusal without
the opt-in.  The criteria are those of tests/test_q32_refined_gpu.py refined_criteria.

LIMIT.  Chosen on the f64 run alone: from 30 down, the first limit at which the f64 solve converges and
rebuilds its D space at least 5 times.  30 is that limit (58 iterations, 48 rebuilds); 2 * nroots = 6 is the
chaotic regime of the reference algorithm and far below.

Measured (this model, dense_3000, 3 roots, 1e-10, limit 30, max_iter 100): the f64 solve converges in 58
iterations with 48 rebuilds; the refined solve in 41 with 10 rebuilds, 30 D-space actions and 66 refined actions
(215 actions in all against 158), its errors equal to the recomputed residual norms.  It rebuilds less often than
the f64 solve because a refined rebuild cuts the Q space two working sets below the limit
(solvers.h refine_dspace_slack): with the reference's schedule -- a rebuild in every iteration -- each rebuild's
rounding of the D parameters takes 2^-24 of the solutions' D part out of the subspace faster than the iterations
restore it, and this solve stalls near 1.6e-10 (errors 7.6e-11, 1.7e-11, 1.6e-10 after 100 iterations).  That
schedule is set_refine_dspace_slack(0), the program's mode dspace0: 100 iterations, 90 rebuilds."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "iterative-solver_amd", "include")]
SAN = os.environ.get("ITSOLV_SAN_FLAGS", "").split()  # tools/asan_cpu.sh: the sanitizer build
EPS = float(np.finfo(np.float64).eps)
N, NROOTS, THRESHOLD, MAX_ITER, LIMIT = 3000, 3, 1e-10, 100, 30


@pytest.fixture(scope="module")
def runs():
    """{"f64", "dspace"} -> the program's JSON line; "refused" -> (return code, stderr); and |H|_2."""
    b = np.random.default_rng(7).uniform(-1, 1, (N, N)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(N), np.arange(N)] = 1 + 9 * np.arange(N) / N
    norm2 = float(np.max(np.abs(np.linalg.eigvalsh(h))))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe, mat = os.path.join(d, "model"), os.path.join(d, "h.bin")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", *SAN, *INC,
                            os.path.join(HERE, "cpp", "q32_refined_dspace_model.cpp"), "-o", exe], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        np.ascontiguousarray(h).tofile(mat)
        # (key, the program's mode, max_p): the _p runs are solve()'s P space of 8 unit vectors
        for key, mode, max_p in (("f64", "f64", 0), ("dspace", "dspace", 0), ("dspace0", "dspace0", 0),
                                 ("refused", "refused", 0), ("f64_p", "f64", 8), ("dspace_p", "dspace", 8)):
            p = subprocess.run([exe, mat, str(N), str(NROOTS), repr(THRESHOLD), str(MAX_ITER), str(LIMIT), mode] +
                               ([str(max_p)] if max_p else []), capture_output=True, text=True, timeout=600)
            if mode == "refused":
                out[key] = (p.returncode, p.stderr)
                continue
            assert p.returncode == 0, p.stderr[-2000:]
            out[key] = json.loads(p.stdout.strip().splitlines()[-1].replace("-nan", "NaN").replace("nan", "NaN"))
            for k in ("eigenvalues", "errors", "residual_norms"):
                out[key][k] = np.array(out[key][k], dtype=float)
    return out, norm2


def test_limit_is_chosen_on_the_f64_run(runs):
    f64 = runs[0]["f64"]
    print(f"\nmodel f64, limit {LIMIT}: iterations {f64['iterations']}, D-space rebuilds {f64['dspace_rebuilds']}")
    assert f64["converged"] and f64["dspace_rebuilds"] >= 5
    assert f64["dspace_actions"] == 0 and f64["refined_actions"] == 0  # no action beyond the solver's own


def test_refined_dspace_model_reaches_1e_10(runs):
    out, norm2 = runs
    f64, ref = out["f64"], out["dspace"]
    recompute = N * EPS * norm2  # worst-case rounding of the recomputed residual: 3.3e-12 here
    print(f"\nmodel dense_3000 at 1e-10, limit {LIMIT}: iterations f64 {f64['iterations']} refined+dspace "
          f"{ref['iterations']} (difference {ref['iterations'] - f64['iterations']}), rebuilds f64 "
          f"{f64['dspace_rebuilds']} refined+dspace {ref['dspace_rebuilds']}, D-space actions {ref['dspace_actions']}, "
          f"refined actions {ref['refined_actions']} of {ref['actions']}, max delta {ref['max_delta']:.3e}\n"
          f"  errors {ref['errors']}\n  residual norms {ref['residual_norms']}\n  f64 residual norms "
          f"{f64['residual_norms']}")
    assert ref["dspace_rebuilds"] >= 5
    assert ref["dspace_actions"] <= NROOTS * ref["dspace_rebuilds"]
    assert f64["converged"] and ref["converged"]
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= THRESHOLD + recompute)
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= recompute)
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])
    assert ref["iterations"] <= f64["iterations"] + 3


def test_dspace_counters_and_eigenvalues(runs):
    """What holds whether or not the last digits of the threshold are reached: the counters, and eigenvalues
    within the sum of the two solves' true residual norms."""
    out, _ = runs
    f64, ref = out["f64"], out["dspace"]
    assert ref["dspace_rebuilds"] >= 5
    assert 1 <= ref["dspace_actions"] <= NROOTS * ref["dspace_rebuilds"]
    # every action beyond the f64 solve's pattern is a refined one or a D-space one
    assert ref["actions"] - ref["refined_actions"] - ref["dspace_actions"] <= NROOTS * ref["iterations"]
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])


def test_refined_dspace_model_with_a_p_space(runs):
    """The same solve with a P space of 8 unit vectors (solve()'s max_p): the P rows of update_dspace_refined
    (S(D,P) and H(P,D) from the twins and their actions against p) and the refined rows of new_qspace_data with
    nP != 0 and nD != 0 together.  Same criteria.  Measured: the f64 solve 46 iterations with 35 rebuilds, the
    refined solve 34 with 7 rebuilds and 21 D-space actions."""
    out, norm2 = runs
    f64, ref = out["f64_p"], out["dspace_p"]
    recompute = N * EPS * norm2
    print(f"\nmodel dense_3000 with max_p = 8, limit {LIMIT}: iterations f64 {f64['iterations']} refined+dspace "
          f"{ref['iterations']}, rebuilds f64 {f64['dspace_rebuilds']} refined+dspace {ref['dspace_rebuilds']}, "
          f"D-space actions {ref['dspace_actions']}\n  errors {ref['errors']}\n  residual norms {ref['residual_norms']}")
    assert f64["converged"] and f64["dspace_rebuilds"] >= 1  # the f64 run alone shows that the limit bites
    assert ref["converged"]
    assert ref["dspace_rebuilds"] >= 1 and 1 <= ref["dspace_actions"] <= NROOTS * ref["dspace_rebuilds"]
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= THRESHOLD + recompute)
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= recompute)
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])
    assert ref["iterations"] <= f64["iterations"] + 3


def test_slack_0_is_the_plain_schedule(runs):
    """set_refine_dspace_slack(0) gives the plain solver's schedule back: once the Q space is full (LIMIT / NROOTS
    iterations) every iteration with a working set rebuilds, as the f64 solve's do.  Whether that solve reaches
    the threshold is not asserted (on this matrix it stalls near 1.6e-10, see above); that the eigenvalues are
    within the two solves' true residual norms is."""
    out, _ = runs
    f64, ref, s0 = out["f64"], out["dspace"], out["dspace0"]
    print(f"\nmodel slack 0: converged {s0['converged']}, iterations {s0['iterations']}, rebuilds "
          f"{s0['dspace_rebuilds']}, D-space actions {s0['dspace_actions']}\n  errors {s0['errors']}\n  residual norms "
          f"{s0['residual_norms']}")
    full = LIMIT // NROOTS  # iterations until the Q space holds LIMIT vectors
    assert s0["dspace_rebuilds"] >= s0["iterations"] - full - 1
    assert s0["dspace_rebuilds"] > ref["dspace_rebuilds"]
    assert 1 <= s0["dspace_actions"] <= NROOTS * s0["dspace_rebuilds"]
    assert np.all(np.abs(s0["eigenvalues"] - f64["eigenvalues"]) <= s0["residual_norms"] + f64["residual_norms"])


def test_limit_without_the_opt_in_is_still_refused(runs):
    code, err = runs[0]["refused"]
    assert code == 1 and "max_size_qspace" in err, err
