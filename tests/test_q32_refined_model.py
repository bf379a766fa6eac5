"""The refined mode of the solver on the CPU (no device): tests/cpp/q32_refined_model.cpp instantiates
LinearEigensystemDavidson<R, Q, P> with R over double storage and Q over float storage, on a minimal handler
of its own with its own quantise_for_storage overload (the restated iterable handlers are typed on
std::vector<double> and do not compile for the pair), and solves the dense_3000 matrix of
tests/test_mixed_gpu.py at 1e-10 with the Q space in f64, in f32 with refinement and in f32 without.

What this exercises: the solver quantising before the action, the refined rows of subspace.h (call by call),
the bound delta and the trigger of refine_residuals.  The criteria are those of the GPU case
(tests/test_q32_refined_gpu.py test_dense_3000_refined_reaches_1e_10)."""
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
    """The three solves of one matrix file: {"f64", "refined", "q32"} -> the program's JSON line; and |H|_2."""
    b = np.random.default_rng(7).uniform(-1, 1, (N, N)) * 0.01
    h = (b + b.T) / 2
    h[np.arange(N), np.arange(N)] = 1 + 9 * np.arange(N) / N
    norm2 = float(np.max(np.abs(np.linalg.eigvalsh(h))))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe, mat = os.path.join(d, "model"), os.path.join(d, "h.bin")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", *SAN, *INC, os.path.join(HERE, "cpp", "q32_refined_model.cpp"),
                            "-o", exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        np.ascontiguousarray(h).tofile(mat)
        for mode in ("f64", "refined", "q32"):
            p = subprocess.run([exe, mat, str(N), str(NROOTS), repr(THRESHOLD), str(MAX_ITER), mode], capture_output=True,
                               text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            out[mode] = json.loads(p.stdout.strip().splitlines()[-1].replace("-nan", "NaN").replace("nan", "NaN"))
            for k in ("eigenvalues", "errors", "residual_norms"):
                out[mode][k] = np.array(out[mode][k], dtype=float)
    return out, norm2


def test_refined_model_reaches_1e_10(runs):
    out, norm2 = runs
    f64, ref = out["f64"], out["refined"]
    recompute = N * EPS * norm2  # worst-case rounding of the recomputed residual: 3.3e-12 here
    print(f"\nmodel dense_3000 at 1e-10: iterations f64 {f64['iterations']} refined {ref['iterations']} (difference "
          f"{ref['iterations'] - f64['iterations']}), refined actions {ref['refined_actions']} of {ref['actions']}, first "
          f"refined iteration {ref['first_refined_iteration']}, max delta {ref['max_delta']:.3e}\n  errors {ref['errors']}\n"
          f"  residual norms {ref['residual_norms']}\n  f64 residual norms {f64['residual_norms']}")
    assert f64["converged"] and ref["converged"]
    for r in (f64, ref):
        assert np.all(r["residual_norms"] <= THRESHOLD + recompute)
    assert np.all(np.abs(ref["errors"] - ref["residual_norms"]) <= recompute)
    assert np.all(np.abs(ref["eigenvalues"] - f64["eigenvalues"]) <= ref["residual_norms"] + f64["residual_norms"])
    assert ref["iterations"] <= f64["iterations"] + 3
    assert 1 <= ref["refined_actions"] <= NROOTS * ref["iterations"]
    assert ref["first_refined_iteration"] >= 2
    # every action beyond the f64 solve's pattern is a refined one: the refined solve's count is the plain
    # per-iteration actions plus the refined actions
    assert ref["actions"] - ref["refined_actions"] <= NROOTS * ref["iterations"]
    assert f64["refined_actions"] == 0 and f64["first_refined_iteration"] == 0


def test_plain_f32_model_does_not_converge_at_1e_10(runs):
    """Passes without the refined mode too: the stall the refined case is measured against."""
    plain = runs[0]["q32"]
    print(f"\nmodel plain f32 Q space at 1e-10: iterations {plain['iterations']}, errors {plain['errors']}")
    assert not plain["converged"] and plain["iterations"] == MAX_ITER
