"""Linear equations with the Q space in f32 on the CPU (no device): tests/cpp/q32_lineq_model.cpp instantiates
LinearEquationsDavidson<R, Q, P> with R over double storage and Q over float storage, on minimal handlers of its
own (the pattern of tests/cpp/q32_refined_model.cpp), and solves the dense_3000 matrix of tests/test_mixed_gpu.py
with 3 right-hand sides from default_rng(11).uniform(-1, 1) at 1e-10: Q in f64, in f32 with refinement, in f32
without, and refined with a P space (max_p = 8).

What this exercises: the twins of the right-hand sides in R's format (subspace.h rhs_r: the subspace rhs rows,
the P rows, construct_residual), the bound delta scaled by 1 / |b| and the trigger of refine_residuals, and the
refusals of LinearEquationsDavidson::check_refine.

Bounds.  A residual norm recomputed in f64 from x carries at most n eps (|A|_2 |x| + |b|) / |b| of rounding
(recompute_r).  For symmetric positive definite A, |x - x*| <= |A x - b| / lambda_min, so two solutions of the
same system differ by at most (res_a + res_b) |b| / lambda_min."""
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
N, NRHS, THRESHOLD, MAX_ITER = 3000, 3, 1e-10, 60
REFUSALS = {"hermitian": "hermitian", "max_size_qspace": "max_size_qspace", "reset_D": "reset_D",
            "reset_D_max_Q_size": "reset_D_max_Q_size", "augmented_hessian": "augmented_hessian",
            "refine_dspace": "refine_dspace"}


def problem():
    b = np.random.default_rng(7).uniform(-1, 1, (N, N)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(N), np.arange(N)] = 1 + 9 * np.arange(N) / N
    rhs = np.random.default_rng(11).uniform(-1, 1, (NRHS, N))
    return h, rhs


@pytest.fixture(scope="module")
def runs():
    """{"f64", "refined", "q32", "refined_p8", "f64_p8"} -> the program's JSON line with "x"; the refusals'
    messages; |A|_2 and lambda_min."""
    h, rhs = problem()
    ev = np.linalg.eigvalsh(h)
    out, refused = {}, {}
    with tempfile.TemporaryDirectory() as d:
        exe, mat, rf = os.path.join(d, "model"), os.path.join(d, "h.bin"), os.path.join(d, "rhs.bin")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", *SAN, *INC, os.path.join(HERE, "cpp", "q32_lineq_model.cpp"),
                            "-o", exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        np.ascontiguousarray(h).tofile(mat)
        np.ascontiguousarray(rhs).tofile(rf)

        def run(mode, max_p=0, max_iter=MAX_ITER, sol=None):
            cmd = [exe, mat, str(N), rf, str(NRHS), repr(THRESHOLD), str(max_iter), str(max_p), mode]
            p = subprocess.run(cmd + ([sol] if sol else []), capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            return json.loads(p.stdout.strip().splitlines()[-1].replace("-nan", "NaN").replace("nan", "NaN"))

        for name, mode, max_p in (("f64", "f64", 0), ("refined", "refined", 0), ("q32", "q32", 0),
                                  ("f64_p8", "f64", 8), ("refined_p8", "refined", 8)):
            sol = os.path.join(d, name + ".x")
            out[name] = run(mode, max_p, sol=sol)
            assert "error" not in out[name], out[name]
            for k in ("errors", "residual_norms", "xnorm", "bnorm"):
                out[name][k] = np.array(out[name][k], dtype=float)
            out[name]["x"] = np.fromfile(sol).reshape(NRHS, N)
        for mode in list(REFUSALS) + ["late"]:
            refused[mode] = run(mode, max_iter=3)
    return out, refused, float(np.max(np.abs(ev))), float(ev[0])


def criteria(name, f64, ref, norm2, lam_min):
    recompute = N * EPS * (norm2 * ref["xnorm"] + ref["bnorm"]) / ref["bnorm"]
    print(f"\n{name}: iterations f64 {f64['iterations']} refined {ref['iterations']}, refined actions "
          f"{ref['refined_actions']} of {ref['actions']}, first refined iteration {ref['first_refined_iteration']}, max delta "
          f"{ref['max_delta']:.3e}\n  errors {ref['errors']}\n  residual norms {ref['residual_norms']}\n  f64 residual norms "
          f"{f64['residual_norms']}\n  recompute {recompute}\n  |x_ref - x_f64| "
          f"{np.linalg.norm(ref['x'] - f64['x'], axis=1)}")
    assert f64["converged"] and ref["converged"]
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= THRESHOLD + recompute)
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= recompute)
    bound = (ref["residual_norms"] + f64["residual_norms"]) * ref["bnorm"] / lam_min
    assert np.all(np.linalg.norm(ref["x"] - f64["x"], axis=1) <= bound)
    assert ref["iterations"] <= f64["iterations"] + 3
    assert 1 <= ref["refined_actions"] <= NRHS * ref["iterations"]
    assert f64["refined_actions"] == 0 and f64["first_refined_iteration"] == 0


def test_refined_model_reaches_1e_10(runs):
    out, _, norm2, lam_min = runs
    assert lam_min > 0
    criteria("model lineq dense_3000 at 1e-10", out["f64"], out["refined"], norm2, lam_min)


def test_refined_model_with_a_p_space(runs):
    """max_p = 8: the P rows of the subspace rhs come from the twins through the R x P handler."""
    out, _, norm2, lam_min = runs
    criteria("model lineq dense_3000 at 1e-10, max_p = 8", out["f64_p8"], out["refined_p8"], norm2, lam_min)


def test_plain_f32_model_does_not_converge_at_1e_10(runs):
    """Passes without the refined mode too: the stall the refined cases are measured against."""
    plain = runs[0]["q32"]
    print(f"\nmodel plain f32 Q space at 1e-10: iterations {plain['iterations']}, errors {plain['errors']}, residual norms "
          f"{plain['residual_norms']}")
    assert not plain["converged"]
    # the rounded right-hand side alone puts the true residual near 2^-24: far above what the solver reports
    assert np.all(plain["residual_norms"] > THRESHOLD)


@pytest.mark.parametrize("mode", sorted(REFUSALS))
def test_refined_mode_refuses_by_name(runs, mode):
    msg = runs[1][mode].get("error", "")
    assert "refine" in msg and REFUSALS[mode] in msg, runs[1][mode]


def test_set_refine_after_add_equations_names_the_fix(runs):
    msg = runs[1]["late"].get("error", "")
    assert "set_refine" in msg and "before add_equations" in msg, runs[1]["late"]
