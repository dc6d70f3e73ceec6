"""Seeded random-shape sweep of the Matern-5/2 Gram operator: matvec and parameter gradients over d, n, p, ARD and arithmetic mode
against the dense torch-fp64 reference of tests/test_gpu_matern52.py.  Shapes and tolerances as tools/fuzz_matvec.py draws and sets
them for Matern-3/2 (line 66: 2e-4 + 2e-4 in "fp32", 2e-4 + 1e-4 in the split modes; gradients, line 83: 5e-3 / 2e-3); a stream
of its own (seed 5252), so no existing sweep is re-drawn."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions.operators import RbfGramOp

from test_gpu_matern52 import DEV, KIND, MINVAL, T, ref_gram

CASES = 36


def draw(case):
    rng = np.random.default_rng([5252, case])
    tier = case % 4
    if tier == 0:
        d, n = int(rng.integers(1, 17)), int(rng.integers(65, 6000))  # split kernels
    elif tier == 1:
        d, n = int(rng.integers(17, 33)), int(rng.integers(65, 5000))  # padded 32
    elif tier == 2:
        d, n = int(rng.integers(33, 129)), int(rng.integers(65, 4000))  # exact-fp32 matrix cores
    else:
        d, n = int(rng.integers(129, 201)), int(rng.integers(65, 2000))  # VALU
    p = int(rng.choice([1, 2, 3, 7, 8, 16, 31, 32, 33, 47, 64, 65, 96, 100]))
    ard = bool(rng.integers(0, 2))
    mode = str(rng.choice(["f16x3", "f16x3-matvec", "fp32"]))
    X = rng.standard_normal((n, d)) * rng.choice([0.3, 1.0, 3.0]) * min(1.0, 4.0 / np.sqrt(d))
    raw = (rng.standard_normal(d) * 0.3 + 0.6 if ard else np.array(0.6 + 0.3 * rng.standard_normal()), np.array(0.3), np.array(-1.0))
    V = rng.standard_normal((p, n)) * np.exp(rng.standard_normal((p, 1)) * 2.0)
    L = rng.standard_normal((p, n))
    return d, n, p, ard, mode, X, raw, V, L


@pytest.mark.parametrize("case", range(CASES))
def test_random_shape(case):
    d, n, p, ard, mode, X, raw, V, L = draw(case)
    X32 = T(X, torch.float32)
    p32 = [T(r, torch.float32, True) for r in raw]
    V32, L32 = T(V, torch.float32), T(L, torch.float32)
    op = RbfGramOp(X32, noise_minval=MINVAL, kernel=KIND, precision=mode)
    y = op(V32, *p32)
    g32 = torch.autograd.grad((L32 * y).sum(), p32)
    p64 = [q.detach().double().requires_grad_(True) for q in p32]
    ref = V32.double() @ ref_gram(X32.double(), p64, float(torch.finfo(torch.float32).eps)).T
    g64 = torch.autograd.grad((L32.double() * ref).sum(), p64)
    err = float(((y.detach().double() - ref.detach()).abs().amax(dim=1) / ref.detach().abs().amax(dim=1)).max())
    tol = 2e-4 + (2e-4 if mode == "fp32" else 1e-4)  # tools/fuzz_matvec.py:66
    print(f"    n={n} d={d} p={p} ard={ard} {mode}: matvec err {err:.2e} (tol {tol:.1e})")
    assert err < tol
    xmax2 = float((X / 0.5).__pow__(2).sum(1).max())
    scale = 1e-7 * float(L32.abs().max() * V32.abs().max()) * n  # tools/fuzz_matvec.py:76-77: the scale of the terms
    gt = 5e-3 if mode == "fp32" else 2e-3  # tools/fuzz_matvec.py:83
    for idx, (a, b) in enumerate(zip(g32, g64)):
        e = float((a.double() - b).abs().max() / (b.abs().max() + scale * (1.0 + xmax2 if idx == 0 else 1.0)))
        print(f"      gradient {('l', 's', 'noise')[idx]} err {e:.2e} (tol {gt:.1e})")
        assert e <= gt
