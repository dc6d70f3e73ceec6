"""Probe groups of the Krylov vector kernels (csrc/mfx_vec.h: Ctx::for_groups) and the adjoint drivers without a start-vector
cotangent (dv == NULL, include/mfx.h).

Grouping launches the same kernels on g probes at a time, so every result must be BIT-IDENTICAL to the ungrouped launch: what can go
wrong is a per-probe pointer that is not offset by the group's first probe (every output and every cotangent below is a per-probe
array), a ragged last group, and a reduction that would cross probes.  The group size is read once per process (MFX_PROBE_GROUP), so
each setting runs in a fresh child process.  Skipping the work behind Lambda[:, 0] must leave the parameter gradients bit-identical,
cost exactly one operator application less, and not touch what dv is when it IS wanted (the oracle, arnoldi.py:104-220).
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import slq_oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, arnoldi, lanczos
    from matfree_extensions.operators import CsrOp, DenseOp, RbfGramOp

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (operator kind, n, d, k, p, forced group size)
CASES = {
    "rbf_ragged": ("rbf", 1003, 3, 6, 5, 2),   # n % 4 != 0: scalar loads; groups of 2, 2 and 1
    "rbf_wide": ("rbf", 4096, 3, 3, 64, 16),   # 16-byte loads, four groups
    "dense": ("dense", 257, 0, 4, 3, 2),
    "csr": ("csr", 257, 0, 4, 3, 2),           # few slices, short rows: the fused step head (launch_csr_step)
}


def _operator(kind, n, d, dtype, seed):
    """-> (operator, parameters that require grad)"""
    rng = np.random.default_rng(seed)
    if kind == "rbf":
        X = torch.tensor(rng.standard_normal((n, d)), dtype=dtype, device=DEV)
        raw = (np.array(0.9), np.array(0.4), np.array(-1.0))
        return RbfGramOp(X, noise_minval=1e-4), [torch.tensor(r, dtype=dtype, device=DEV, requires_grad=True) for r in raw]
    if kind == "dense":
        A = np.eye(n) * 2.0 + rng.standard_normal((n, n)) / np.sqrt(n)
        A = 0.5 * (A + A.T)
        return DenseOp(), [torch.tensor(A, dtype=dtype, device=DEV, requires_grad=True)]
    r, c, vals, n2 = orc.laplacian_2d_plus_identity(16)
    assert n2 == 256
    r, c = np.concatenate([r, [256]]), np.concatenate([c, [256]])  # one more unknown: n = 257
    vals = np.concatenate([vals, [3.0]])
    op, vt, _order = CsrOp.from_coo(r, c, vals, n, DEV)
    return op, [vt.to(dtype).requires_grad_(True)]


def _outputs(name, dtype=torch.float32):
    """Forward outputs and, under a random cotangent for EVERY output, all gradients: Arnoldi with both adjoint re-projection
    modes and the three-term Lanczos recurrence."""
    kind, n, d, k, p, _g = CASES[name]
    op, params = _operator(kind, n, d, dtype, seed=n + p)
    gen = torch.Generator().manual_seed(n)
    V = torch.randn((p, n), generator=gen, dtype=dtype).to(DEV).requires_grad_(True)
    out = {}

    def cotangents(ts):
        return [torch.randn(t.shape, generator=gen, dtype=dtype).to(DEV) for t in ts]

    for reortho in ("full", "none"):
        res = arnoldi.hessenberg(op, k, reortho=reortho)(V, *params)
        grads = torch.autograd.grad(res, (V, *params), cotangents(res))
        for nm, t in zip(("Q", "H", "r", "c", "dv", *[f"dp{i}" for i in range(len(params))]), (*res, *grads)):
            out[f"arnoldi_{reortho}_{nm}"] = t.detach().contiguous().cpu()
    (basis, (diag, off)), (q, b) = lanczos.tridiag(op, k, reortho="none")(V / V.norm(dim=-1, keepdim=True), *params)
    res = (basis, diag, off, q, b)
    grads = torch.autograd.grad(res, (V, *params), cotangents(res))
    for nm, t in zip(("xs", "alpha", "beta", "q", "b", "dv", *[f"dp{i}" for i in range(len(params))]), (*res, *grads)):
        out[f"lanczos_{nm}"] = t.detach().contiguous().cpu()
    return out


CHILD = r"""
import sys, torch
sys.path.insert(0, {tests!r})
sys.path.insert(0, {root!r})
sys.path.insert(0, {pkg!r})
import test_gpu_probe_groups as t
torch.save(t._outputs({name!r}), {out!r})
print("child ok")
"""


def _run_child(tmp_path, name, group):
    out = str(tmp_path / f"{name}_g{group}.pt")
    root = os.path.dirname(HERE)
    code = CHILD.format(tests=HERE, root=root, pkg=os.path.join(root, "experiments-lanczos-adjoints_amd"), name=name, out=out)
    env = dict(os.environ, MFX_PROBE_GROUP=str(group))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return torch.load(out)


@pytest.mark.parametrize("name", list(CASES))
def test_grouped_equals_ungrouped_bitwise(tmp_path, name):
    whole = _run_child(tmp_path, name, 0)
    grouped = _run_child(tmp_path, name, CASES[name][5])
    assert set(whole) == set(grouped) and len(whole) >= 19
    for key, ref in whole.items():
        assert torch.isfinite(ref).all(), key
        assert torch.equal(grouped[key], ref), (name, key, (grouped[key] - ref).abs().max().item())


# ------------------------------------------------------------------------------------------------------------------------
# dv == NULL: the adjoint without the cotangent of the start vector
# ------------------------------------------------------------------------------------------------------------------------
def _arnoldi_grads(op, k, V, params, cot, reortho="full"):
    """-> (gradients in the order (V if it requires grad, *params), operator applications the backward pass issued)"""
    res = arnoldi.hessenberg(op, k, reortho=reortho)(V, *params)
    wrt = ([V] if V.requires_grad else []) + list(params)
    torch.cuda.synchronize()
    _lib.timing_reset()
    _lib.timing_enable(True)
    try:
        grads = torch.autograd.grad(res, wrt, cot)
        torch.cuda.synchronize()
        _ms, applications = _lib.timing_read(0)
    finally:
        _lib.timing_enable(False)
        _lib.timing_reset()
    return res, grads, applications


@pytest.mark.parametrize("dtype,gtol", [(torch.float64, 1e-7), (torch.float32, 5e-3)])  # tests/test_gpu_parity.py::test_arnoldi_adjoint_golden
def test_adjoint_without_start_vector_cotangent(dtype, gtol):
    _kind, n, d, k, p, _g = CASES["rbf_ragged"]
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, d))
    raw = (np.array(0.9), np.array(0.4), np.array(-1.0))
    v = rng.standard_normal((p, n))
    op = RbfGramOp(torch.tensor(X, dtype=dtype, device=DEV), noise_minval=1e-4)
    params = [torch.tensor(r, dtype=dtype, device=DEV, requires_grad=True) for r in raw]
    o = orc.RbfGramOp(X, noise_minval=1e-4, eps=float(torch.finfo(dtype).eps))
    fwd = [orc.arnoldi_forward(o, k, v[b], *raw, reortho="full") for b in range(p)]
    cot_np = [np.stack([rng.standard_normal(np.shape(f[i])) for f in fwd]) for i in range(4)]
    cot = [torch.tensor(x, dtype=dtype, device=DEV) for x in cot_np]

    V = torch.tensor(v, dtype=dtype, device=DEV)
    _, without, n_without = _arnoldi_grads(op, k, V, params, cot)
    _, with_dv, n_with = _arnoldi_grads(op, k, V.clone().requires_grad_(True), params, cot)
    assert (n_without, n_with) == (k - 1, k)
    for a, b in zip(without, with_dv[1:]):
        assert torch.equal(a, b)
    # dv, when it is wanted, is what the reference's algorithm gives
    for b in range(p):
        Qo, Ho, ro, co = fwd[b]
        dv_o, _dp = orc.arnoldi_adjoint(o, raw, Q=Qo, H=Ho, r=ro, c=co, dQ=cot_np[0][b], dH=cot_np[1][b], dr=cot_np[2][b],
                                        dc=float(cot_np[3][b]), reortho="full")
        got = with_dv[0][b].detach().cpu().numpy().astype(np.float64)
        assert np.allclose(got, dv_o, rtol=gtol, atol=gtol * np.abs(dv_o).max()), (b, np.abs(got - dv_o).max(), np.abs(dv_o).max())


def test_three_term_adjoint_without_start_vector_cotangent():
    _kind, n, d, k, p, _g = CASES["rbf_ragged"]
    op, params = _operator("rbf", n, d, torch.float32, seed=7)
    gen = torch.Generator().manual_seed(7)
    V = torch.randn((p, n), generator=gen).to(DEV)
    V = V / V.norm(dim=-1, keepdim=True)
    grads, counts = [], []
    for wanted in (False, True):
        Vin = V.clone().requires_grad_(wanted)
        (basis, (diag, off)), (q, b) = lanczos.tridiag(op, k, reortho="none")(Vin, *params)
        g2 = torch.Generator().manual_seed(8)
        cot = [torch.randn(t.shape, generator=g2).to(DEV) for t in (basis, diag, off, q, b)]
        torch.cuda.synchronize()
        _lib.timing_reset()
        _lib.timing_enable(True)
        try:
            grads.append(torch.autograd.grad((basis, diag, off, q, b), ([Vin] if wanted else []) + params, cot))
            torch.cuda.synchronize()
            counts.append(_lib.timing_read(0)[1])
        finally:
            _lib.timing_enable(False)
            _lib.timing_reset()
    assert counts == [k - 1, k]
    for a, b in zip(grads[0], grads[1][1:]):
        assert torch.equal(a, b)


def test_callback_operator_is_still_applied_k_times():
    """A callback operator accumulates its parameter gradient inside every application (arnoldi.py:207-209): none is skipped."""
    n, k, p = 257, 4, 3
    rng = np.random.default_rng(1)
    A0 = np.eye(n) * 2.0 + rng.standard_normal((n, n)) / np.sqrt(n)
    A = torch.tensor(A0, dtype=torch.float64, device=DEV, requires_grad=True)
    V = torch.tensor(rng.standard_normal((p, n)), dtype=torch.float64, device=DEV)
    calls = []

    def matvec(s, a):
        calls.append(1)
        return a @ s

    results = []
    for wanted in (False, True):
        Vin = V.clone().requires_grad_(wanted)
        res = arnoldi.hessenberg(matvec, k, reortho="full")(Vin, A)
        gen = torch.Generator().manual_seed(2)
        cot = [torch.randn(t.shape, generator=gen, dtype=torch.float64).to(DEV) for t in res]
        del calls[:]
        g = torch.autograd.grad(res, ([Vin] if wanted else []) + [A], cot)
        results.append((len(calls), g[-1]))
    assert results[0][0] == results[1][0] == k * p  # one call per probe and application
    assert torch.equal(results[0][1], results[1][1])
    # and against the native operator, which does skip: the same parameter gradient
    res = arnoldi.hessenberg(DenseOp(), k, reortho="full")(V, A)
    gen = torch.Generator().manual_seed(2)
    cot = [torch.randn(t.shape, generator=gen, dtype=torch.float64).to(DEV) for t in res]
    (dA,) = torch.autograd.grad(res, [A], cot)
    assert torch.allclose(dA, results[0][1], rtol=1e-9, atol=1e-11 * dA.abs().max().item())
