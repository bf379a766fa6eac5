"""The refined mode driven by hand on the CPU (no device), as the reverse-communication API drives it:
tests/cpp/rc_refine_model.cpp runs LinearEigensystemDavidson<R over double, Q over float> through quantise,
action, add_vector, precondition, end_iteration -- never solve() -- with the refined residuals' action given
by set_refine_action, on the dense_3000 matrix of tests/test_mixed_gpu.py at 1e-10.

The criteria are those of tests/test_q32_refined_model.py::test_refined_model_reaches_1e_10; the same loop
without set_refine must not converge in 60 iterations; and with set_refine but no action the needed
refinement is an error that names set_refine_action and the C call."""
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
N, NROOTS, THRESHOLD, MAX_ITER = 3000, 3, 1e-10, 60


@pytest.fixture(scope="module")
def runs():
    """{"f64", "refined", "q32"} -> the program's JSON line; "noaction" -> (exit status, stderr); and |H|_2."""
    b = np.random.default_rng(7).uniform(-1, 1, (N, N)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(N), np.arange(N)] = 1 + 9 * np.arange(N) / N
    norm2 = float(np.max(np.abs(np.linalg.eigvalsh(h))))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe, mat = os.path.join(d, "model"), os.path.join(d, "h.bin")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", *SAN, *INC, os.path.join(HERE, "cpp", "rc_refine_model.cpp"),
                            "-o", exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        np.ascontiguousarray(h).tofile(mat)
        for mode in ("f64", "refined", "q32", "noaction"):
            p = subprocess.run([exe, mat, str(N), str(NROOTS), repr(THRESHOLD), str(MAX_ITER), mode], capture_output=True,
                               text=True, timeout=600)
            if mode == "noaction":
                out[mode] = (p.returncode, p.stderr)
                continue
            assert p.returncode == 0, p.stderr[-2000:]
            out[mode] = json.loads(p.stdout.strip().splitlines()[-1].replace("-nan", "NaN").replace("nan", "NaN"))
            for k in ("eigenvalues", "errors", "residual_norms"):
                out[mode][k] = np.array(out[mode][k], dtype=float)
    return out, norm2


def test_hand_driven_refined_model_reaches_1e_10(runs):
    out, norm2 = runs
    f64, ref = out["f64"], out["refined"]
    recompute = N * EPS * norm2  # worst-case rounding of the recomputed residual: 3.3e-12 here
    print(f"\nhand-driven model dense_3000 at 1e-10: iterations f64 {f64['iterations']} refined {ref['iterations']} "
          f"(difference {ref['iterations'] - f64['iterations']}), refined actions {ref['refined_actions']} of "
          f"{ref['actions']}, first refined iteration {ref['first_refined_iteration']}, max delta {ref['max_delta']:.3e}\n"
          f"  errors {ref['errors']}\n  residual norms {ref['residual_norms']}\n  f64 residual norms {f64['residual_norms']}")
    assert f64["converged"] and ref["converged"]
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= THRESHOLD + recompute)
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= recompute)
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])
    assert ref["iterations"] <= f64["iterations"] + 3
    assert 1 <= ref["refined_actions"] <= NROOTS * ref["iterations"]
    assert ref["first_refined_iteration"] >= 2
    assert ref["actions"] - ref["refined_actions"] <= NROOTS * ref["iterations"]
    assert f64["refined_actions"] == 0 and f64["first_refined_iteration"] == 0


def test_the_same_loop_without_set_refine_does_not_converge(runs):
    plain = runs[0]["q32"]
    print(f"\nhand-driven plain f32 Q space at 1e-10: iterations {plain['iterations']}, errors {plain['errors']}")
    # it stalls: either the iterations run out, or the working set empties (every new direction is redundant at
    # the f32 level) with residuals still above the threshold
    assert not plain["converged"] and plain["iterations"] <= MAX_ITER and np.max(plain["errors"]) > THRESHOLD


def test_a_needed_refinement_without_an_action_names_the_calls_that_give_it(runs):
    code, err = runs[0]["noaction"]
    assert code == 3, (code, err)
    assert "set_refine_action" in err and "IterativeSolverHbmSetRefineAction" in err, err
