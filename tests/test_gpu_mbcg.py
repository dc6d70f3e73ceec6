"""Modified batched CG on the GPU (mfx_mbcg_solve, mfx_precond_sample, cg.mbcg_*, gp_util.krylov_logdet_mbcg / logpdf_mbcg) against
mfx_pcg_solve (bitwise), the NumPy restatement of tests/_mbcg_restatement.py (coefficients) and dense fp64 expressions computed from
the SAME probes (value and gradient: no Monte-Carlo tolerance anywhere).

Tolerances are the parity rules of SURVEY.md section 8(d): fp64 forward 1e-9, fp64 gradients 1e-7, fp32 value 1e-4, fp32 gradients
rtol 1e-3 with atol 1e-5 |g|_inf against the fp64 run."""

import ctypes
import functools
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mbcg_restatement as mb
from matfree_extensions import _lib, cg, hutchinson, low_rank
from matfree_extensions.operators import CallbackOp, DenseOp, RbfGramOp, RowShardedOp
from matfree_extensions.util import gp_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TRAIN = os.path.join(ROOT, "experiments", "applications", "gaussian_process", "train", "optim_logml_mbcg_adaptive.py")
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64


def _inv_softplus(v):
    return math.log(math.expm1(v))


def _np(t):
    return t.detach().double().cpu().numpy()


def _rbf_problem(n, dtype, rank, seed=0, precision="f16x3", lengthscale=1.0, noise=0.1):
    """RBF Gram operator (d = 3, outputscale 1, the given lengthscale and noise; the defaults are the table's setting), its pivoted
    rank-`rank` preconditioner bound to the noise (None for rank 0), and the same matrices in fp64 NumPy, built from the values the
    device holds."""
    rng = np.random.default_rng(seed)
    X = torch.tensor(rng.standard_normal((n, 3)), dtype=dtype, device=DEV)
    raw = [torch.tensor(_inv_softplus(v), dtype=dtype, device=DEV) for v in (lengthscale, 1.0, noise)]
    op = RbfGramOp(X, noise_minval=0.0, precision=precision)
    A = op.bind(*raw)
    ls, s, nz = (float(_np(q)[0]) for q in op.constrain(*raw))
    A_np = mb.rbf_gram(_np(X), ls, s, nz)
    P, L_np, M_np = None, None, None
    if rank:
        pre, info = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank))(low_rank.without_noise(A), n)
        assert bool(info["success"])
        P = pre.bind(torch.tensor(nz, dtype=dtype, device=DEV))
        L_np = _np(pre.lt).T.copy()
        M_np = float(_np(P.s)) * np.eye(n) + L_np @ L_np.T
    return A, P, A_np, L_np, M_np


def _cfg(mode, maxiter=12):
    if mode == "fixed":
        return cg.mbcg_fixed_step(maxiter), None
    return cg.mbcg_adaptive(atol=3e-2, rtol=0.0, maxiter=maxiter, miniter=2), (3e-2, 0.0, 2)


# The operator of the bitwise / coefficient / padding cases: lengthscale 0.5, noise 0.5.  Twelve CG steps amplify a rounding-level
# difference between two correct implementations by a factor that depends on the spectrum: perturbing the matvec of the NumPy
# restatement by 1e-16 moves ITS OWN coefficients by 3.5e-11 at (lengthscale 1, noise 0.1, n = 2050) -- too close to the 1e-9 of the
# coefficient check for a device reduction order that differs by 1e-15 -- and by 9e-16 at (0.5, 0.5), where the check is sharp.
WELL = dict(lengthscale=0.5, noise=0.5)

CASES = [(n, dtype, rank, mode) for n in (70, 2050) for dtype in (F32, F64) for rank in (0, 5) for mode in ("fixed", "adaptive")]


@functools.lru_cache(maxsize=None)
def _solved(n, dtype, rank, mode):
    A, P, A_np, L_np, M_np = _rbf_problem(n, dtype, rank, **WELL)
    B = torch.tensor(np.random.default_rng(1).standard_normal((4, n)), dtype=dtype, device=DEV)
    solve, adaptive = _cfg(mode)
    x, info = solve(A, B, P)
    plain = {k: v for k, v in solve.cfg.items() if k != "mbcg"}
    ref = cg._solve(A, B, P, plain)  # mfx_pcg_solve
    torch.cuda.synchronize()
    return (A, P, A_np, L_np, M_np, B, adaptive), (x, info), ref


# ---- 1. bitwise with PCG -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype,rank,mode", CASES)
def test_solution_residual_and_steps_are_those_of_pcg_bitwise(n, dtype, rank, mode):
    _, (x, info), (x_ref, r_ref, steps_ref) = _solved(n, dtype, rank, mode)
    assert torch.equal(x, x_ref) and torch.equal(info["residual_abs"], r_ref) and torch.equal(info["num_steps"], steps_ref)
    assert torch.isfinite(x).all() and x.abs().max() > 0


# ---- 2. coefficients (fp64) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype,rank,mode", [c for c in CASES if c[1] is F64])
def test_coefficients_match_the_restatement(n, dtype, rank, mode):
    (A, P, A_np, L_np, M_np, B, adaptive), (x, info), _ = _solved(n, dtype, rank, mode)
    precond = mb.woodbury(L_np, float(_np(P.s)), np.float64) if rank else None
    x_r, r_r, steps_r, rzs, paps, w0_r = mb.pcg(A_np, _np(B), precond, 12, adaptive)
    tdiag_r, toff_r, depth_r = mb.tridiag(rzs, paps, steps_r, 12)
    tdiag, toff = (_np(t) for t in info["tridiag"])
    assert np.array_equal(info["num_steps"].cpu().numpy(), steps_r)
    assert np.array_equal(info["depth"].cpu().numpy(), depth_r) and depth_r.max() > 1
    for name, got, want in (("tdiag", tdiag, tdiag_r), ("toff", toff, toff_r), ("rz0", _np(info["rz0"]), rzs[:, 0]),
                            ("w0", _np(info["w0"]), w0_r)):
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name}: max error / max {err:.2e}")
        assert np.allclose(got, want, rtol=1e-9, atol=0.0), (name, np.abs(got - want).max())
    for b, m in enumerate(depth_r):  # the padding is exact
        assert np.all(tdiag[b, m:] == 1.0) and np.all(toff[b, max(m - 1, 0):] == 0.0)


# ---- 3. padding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_a_zero_right_hand_side_is_the_identity_block(dtype):
    A, P, *_ = _rbf_problem(70, dtype, 5, **WELL)
    B = torch.tensor(np.random.default_rng(2).standard_normal((3, 70)), dtype=dtype, device=DEV)
    B[1] = 0.0
    x, info = cg.mbcg_fixed_step(12)(A, B, P)
    tdiag, toff = info["tridiag"]
    assert info["depth"].tolist() == [12, 0, 12] and info["rz0"][1] == 0
    assert torch.all(tdiag[1] == 1) and torch.all(toff[1] == 0) and torch.all(x[1] == 0) and torch.all(info["w0"][1] == 0)
    for t in (x, info["residual_abs"], tdiag, toff, info["rz0"], info["w0"]):
        assert torch.isfinite(t).all()
    quad = gp_util._mbcg_quadrature(tdiag, toff, info["rz0"])
    assert quad[1] == 0 and torch.isfinite(quad).all()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_a_column_that_never_iterates_has_depth_zero(dtype):
    A, P, *_ = _rbf_problem(70, dtype, 0, **WELL)
    b1 = torch.tensor(np.random.default_rng(3).standard_normal(70), dtype=dtype, device=DEV)
    B = torch.stack([b1, 1e-6 * b1])
    x, info = cg.mbcg_adaptive(atol=1e-3, rtol=0.0, maxiter=12, miniter=0)(A, B, P)
    steps, depth = info["num_steps"].tolist(), info["depth"].tolist()
    assert steps[1] == 0 and depth[1] == 0 and steps[0] >= 2 and depth[0] == steps[0]
    tdiag, toff = info["tridiag"]
    for b, m in enumerate(depth):
        assert torch.all(tdiag[b, m:] == 1) and torch.all(toff[b, max(m - 1, 0):] == 0)
        assert torch.all(tdiag[b, :m] > 0) and torch.all(toff[b, : max(m - 1, 0)] > 0)
    assert torch.all(x[1] == 0) and torch.equal(info["w0"], B)  # no preconditioner: w0 is a copy of b


def test_three_distinct_eigenvalues_run_past_convergence():
    """fixed-step maxiter = n = 40 on a dense SPD matrix with three distinct eigenvalues: CG converges in three steps and keeps
    iterating on round-off until the live-step rule stops the tridiagonal; the quadrature is b^T log(A) b"""
    n = 40
    rng = np.random.default_rng(4)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.repeat([0.5, 2.0, 9.0], [13, 13, 14])
    A_np = (Q * lam) @ Q.T
    A_np = 0.5 * (A_np + A_np.T)
    B_np = rng.standard_normal((3, n))
    x, info = cg.mbcg_fixed_step(n)(DenseOp().bind(torch.tensor(A_np, device=DEV)), torch.tensor(B_np, device=DEV), None)
    tdiag, toff = info["tridiag"]
    for t in (x, info["residual_abs"], tdiag, toff, info["rz0"]):
        assert torch.isfinite(t).all()
    depth = info["depth"].tolist()
    assert all(3 <= m <= n for m in depth), depth
    got = _np(gp_util._mbcg_quadrature(tdiag, toff, info["rz0"]))
    want = mb.dense_quadform(A_np, None, B_np)
    print("depth", depth, "relative errors", np.abs(got - want) / np.abs(want))
    assert np.allclose(got, want, rtol=1e-10, atol=0.0), (got, want)


# ---- 4. value ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [0, 8])
@pytest.mark.parametrize("dtype,precision,tol", [(F64, "fp32", 1e-9), (F32, "f16x3", 1e-4), (F32, "fp32", 1e-4)])
def test_logdet_equals_the_dense_expression_from_the_same_probes(dtype, precision, tol, rank):
    n, p, seed = 96, 4, 11
    A, P, A_np, L_np, M_np = _rbf_problem(n, dtype, rank, precision=precision)
    logdet = gp_util.krylov_logdet_mbcg(cg.mbcg_fixed_step(n), num_probes=p)
    value, info = logdet(A, seed, P)
    if rank:
        z = P.sample(seed, p)
        want = np.linalg.slogdet(M_np)[1] + mb.dense_quadform(A_np, M_np, _np(z)).mean()
    else:
        z = hutchinson.sampler_rademacher(torch.empty(n, dtype=dtype, device=DEV), num=p)(seed)
        want = mb.dense_quadform(A_np, None, _np(z)).mean()
    err = abs(float(value) - want) / abs(want)
    print(f"{dtype} {precision} rank {rank}: value {float(value):.12g} dense {want:.12g} rel {err:.2e} depth {info['solve']['depth'].tolist()}")
    assert err <= tol, (float(value), want)
    again, _ = logdet(A, z, P)  # explicit probes: the same numbers
    assert float(again) == float(value)


# ---- 5. sampler ----------------------------------------------------------------------------------------------------------------
def _sample(dtype, n, rank, lt, shift, seed, first, p):
    out = torch.empty((p, n), dtype=dtype, device=DEV)
    _lib.check(_lib.get().mfx_precond_sample(_lib.dtype_code(dtype), n, rank, _lib.ptr(lt), _lib.ptr(shift), seed, first, p,
                                             _lib.ptr(out), _lib.stream_ptr(DEV)))
    return out


@pytest.mark.parametrize("n,p,rank", [(70, 4, 5), (2050, 4, 5), (333, 11, 3)])
@pytest.mark.parametrize("dtype,rtol", [(F64, 1e-12), (F32, 1e-5)])
def test_sampler_is_the_rademacher_probe_through_the_factor(dtype, rtol, n, p, rank):
    """sqrt(s) R[:, :n] + R[:, n:] @ Lt with R the (p, n + rank) probe of mfx_rademacher.  The order of the sum over c is free, so the
    factor is chosen such that no element can cancel (sqrt(s) = 4 against sum_c |Lt[c][i]| <= 4/3): an elementwise rtol then bounds the
    rounding of the sum itself.  p = 11 spans two probe blocks of the kernel."""
    seed, first, s = 99, 3, 16.0
    rng = np.random.default_rng(5)
    lt = torch.tensor(rng.uniform(-1.0, 1.0, (rank, n)) * 4.0 ** -np.arange(rank)[:, None], dtype=dtype, device=DEV)
    shift = torch.tensor([s], dtype=dtype, device=DEV)
    got = _sample(dtype, n, rank, lt, shift, seed, first, p)
    R = _np(hutchinson.sampler_rademacher(torch.empty(n + rank, dtype=dtype, device=DEV), num=p)((seed, first)))
    want = math.sqrt(s) * R[:, :n] + R[:, n:] @ _np(lt)
    assert np.allclose(_np(got), want, rtol=rtol, atol=0.0), np.abs(_np(got) / want - 1).max()
    # two calls tile one probe matrix
    if p == 4:
        halves = torch.cat([_sample(dtype, n, rank, lt, shift, seed, first, 2), _sample(dtype, n, rank, lt, shift, seed, first + 2, 2)])
        assert torch.equal(halves, got)
    pre = low_rank.Preconditioner(lt.t())
    assert torch.equal(pre.sample(seed, p, s, first_probe=first), got)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n,p", [(70, 4), (2050, 11)])
def test_sampler_without_a_factor_is_mfx_rademacher_bitwise(dtype, n, p):
    got = _sample(dtype, n, 0, None, None, 5, 2, p)
    want = hutchinson.sampler_rademacher(torch.empty(n, dtype=dtype, device=DEV), num=p)((5, 2))
    assert torch.equal(got, want) and set(got.unique().tolist()) == {-1.0, 1.0}
    halves = torch.cat([_sample(dtype, n, 0, None, None, 5, 0, 2), _sample(dtype, n, 0, None, None, 5, 2, 2)])
    assert torch.equal(halves, _sample(dtype, n, 0, None, None, 5, 0, 4))


# ---- 6. gradient ---------------------------------------------------------------------------------------------------------------
def _dense_cov(kind, X, raw_l, raw_s, raw_n):
    """K(X, X) + noise I in plain torch, as the native operator defines it: inputs divided by the lengthscale, the distance of a point
    to itself exactly 0, eps of the dtype under Matern's square root."""
    ls, s, nz = (torch.nn.functional.softplus(q) for q in (raw_l, raw_s, raw_n))
    Xs = X / ls
    diff = Xs[:, None, :] - Xs[None, :, :]
    dist = (diff * diff).sum(-1)
    if kind == "rbf":
        K = torch.exp(-0.5 * dist)
    else:
        r = torch.sqrt(3.0 * dist + torch.finfo(X.dtype).eps)
        K = (1 + r) * torch.exp(-r)
    return s * K + nz * torch.eye(X.shape[0], dtype=X.dtype, device=X.device)


GRAD_CASES = [("matern32", True, 0, False), ("matern32", True, 8, True), ("rbf", False, 0, False), ("rbf", False, 8, False)]


def _gp_setup(kind, ard, dtype, xgrad, n=96, d=3, seed=6):
    rng = np.random.default_rng(seed)
    X = torch.tensor(rng.standard_normal((n, d)), dtype=dtype, device=DEV, requires_grad=xgrad)
    y = torch.tensor(np.sin(rng.standard_normal(n)) + 0.3, dtype=dtype, device=DEV, requires_grad=True)
    raw_l = torch.tensor(rng.uniform(0.3, 0.9, d) if ard else 0.6, dtype=dtype, device=DEV, requires_grad=True)
    raw_s = torch.tensor(0.4, dtype=dtype, device=DEV, requires_grad=True)
    raw_n = torch.tensor(_inv_softplus(0.1), dtype=dtype, device=DEV, requires_grad=True)
    const = torch.tensor(0.2, dtype=dtype, device=DEV, requires_grad=True)
    return X, y, raw_l, raw_s, raw_n, const


@functools.lru_cache(maxsize=None)
def _mbcg_gradients(kind, ard, rank, xgrad, dtype):
    """value and gradients of logpdf_mbcg (w.r.t. raw lengthscale, outputscale, noise, the mean constant, y and, when asked, X), and
    what the dense reference needs: the leaves, the probes and the preconditioner's matrix.

    The fp32 run takes the FACTOR of the fp64 run, cast: both runs then estimate with the same preconditioner and the same probes
    z = sqrt(s) e_1 + L e_2.  A factor computed in fp32 is another matrix whenever two residual diagonals tie below fp32 resolution
    (Matern-3/2 ARD case: the second pivot wins by 9e-9 relative; fp64 picks rows 0, 50, 75, .. and fp32 rows 0, 49, 36, ..), and two
    4-probe estimates with different M and z differ by their Monte-Carlo error, which no rounding tolerance describes."""
    n, p, seed = 96, 4, 21
    X, y, raw_l, raw_s, raw_n, const = _gp_setup(kind, ard, dtype, xgrad)
    op = RbfGramOp(X, noise_minval=0.0, kernel=kind)
    cov = op.bind(raw_l, raw_s, raw_n)
    P, M = None, None
    if rank:
        if dtype is F64:
            pre, _ = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank))(low_rank.without_noise(cov), n)
        else:
            pre = low_rank.Preconditioner(_mbcg_gradients(kind, ard, rank, xgrad, F64)[5].t().to(dtype))
        P = pre.bind(torch.nn.functional.softplus(raw_n))
        z = P.sample(seed, p)
        L = pre.lt.double().t()
        M = float(_np(P.s)) * torch.eye(n, dtype=F64, device=DEV) + L @ L.t()
    else:
        z = hutchinson.sampler_rademacher(torch.empty(n, dtype=dtype, device=DEV), num=p)(seed)
    logpdf = gp_util.logpdf_mbcg(cg.mbcg_fixed_step(n), num_probes=p)
    value, info = logpdf(y, seed, mean=const.expand(n), cov_matvec=cov, P=P)
    leaves = [raw_l, raw_s, raw_n, const, y] + ([X] if xgrad else [])
    grads = torch.autograd.grad(value, leaves)
    return value.detach(), [g.detach() for g in grads], leaves, z, M, (pre.lt if rank else None)


@pytest.mark.parametrize("kind,ard,rank,xgrad", GRAD_CASES)
def test_gradients_equal_autograd_of_the_dense_surrogate(kind, ard, rank, xgrad):
    """d logpdf = d [-alpha^T (y - m) + 1/2 alpha^T A(theta) alpha - 1/(2p) sum_b x_b^T A(theta) w_b] with alpha = A^-1 (y - m),
    x_b = A^-1 z_b, w_b = M^-1 z_b detached and computed densely from the same z (the first term carries the gradients of y and the
    mean, which the parameter surrogate alone does not have)."""
    value, grads, leaves, z, M, _lt = _mbcg_gradients(kind, ard, rank, xgrad, F64)
    raw_l, raw_s, raw_n, const, y = leaves[:5]
    X = leaves[5] if xgrad else _gp_setup(kind, ard, F64, False)[0]
    p = z.shape[0]
    A = _dense_cov(kind, X, raw_l, raw_s, raw_n)
    resid = y - const
    with torch.no_grad():
        alpha = torch.linalg.solve(A, resid)
        xs = torch.linalg.solve(A, z.t()).t()
        ws = z if M is None else torch.linalg.solve(M, z.t()).t()
        logdet = torch.linalg.slogdet(A)[1]
    surrogate = -(alpha @ resid) + 0.5 * alpha @ (A @ alpha) - 0.5 / p * ((xs @ A) * ws).sum()
    want = torch.autograd.grad(surrogate, leaves)
    for name, g, w in zip(("raw_lengthscale", "raw_outputscale", "raw_noise", "mean", "y", "X"), grads, want):
        g, w = _np(g), _np(w)
        print(f"{name}: max |g - w| / max |w| = {np.abs(g - w).max() / np.abs(w).max():.2e}")
        assert np.allclose(g, w, rtol=1e-7, atol=0.0), (name, g, w)
    # the value beside it: the Mahalanobis term exact, the log-determinant an estimate from p = 4 probes (sanity only, no tolerance of its own)
    exact = -0.5 * float(resid.detach() @ alpha) - 0.5 * float(logdet) - 96 / 2 * math.log(2 * math.pi)
    assert math.isfinite(float(value)) and abs(float(value) - exact) < 0.5 * abs(exact)


@pytest.mark.parametrize("kind,ard,rank,xgrad", GRAD_CASES)
def test_fp32_gradients_against_the_fp64_run(kind, ard, rank, xgrad):
    _, g64, *_ = _mbcg_gradients(kind, ard, rank, xgrad, F64)
    _, g32, *_ = _mbcg_gradients(kind, ard, rank, xgrad, F32)
    for name, g, w in zip(("raw_lengthscale", "raw_outputscale", "raw_noise", "mean", "y", "X"), g32, g64):
        g, w = _np(g), _np(w)
        print(f"{name}: max |g - w| / max |w| = {np.abs(g - w).max() / np.abs(w).max():.2e}")
        assert np.allclose(g, w, rtol=1e-3, atol=1e-5 * np.abs(w).max()), (name, g, w)


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preconditioned", [True, False])
def test_target_logml_end_to_end(preconditioned):
    n, d, p, seed, rank = 256, 4, 4, 31, 10
    rng = np.random.default_rng(7)
    X = torch.tensor(rng.standard_normal((n, d)), dtype=F64, device=DEV)
    y = torch.tensor(np.sin(_np(X) @ rng.standard_normal(d)) + 0.1 * rng.standard_normal(n), dtype=F64, device=DEV)
    constrain = gp_util.constraint_greater_than(1e-4)
    m, _ = gp_util.mean_constant(shape_out=())
    k, _ = gp_util.kernel_scaled_matern_32(shape_in=(d,), shape_out=())
    prior = gp_util.model_gp(m, k)
    logpdf = gp_util.logpdf_mbcg(cg.mbcg_fixed_step(n), num_probes=p)
    precondition = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank))
    if preconditioned:
        likelihood, _ = gp_util.likelihood_pdf_p(gp_util.gram_matvec(), logpdf, precondition, constrain=constrain)
    else:
        likelihood, _ = gp_util.likelihood_pdf(gp_util.gram_matvec(), logpdf, constrain=constrain)
    leaf = lambda v: torch.tensor(v, dtype=F64, device=DEV, requires_grad=True)  # noqa: E731
    params = ({"constant_value": leaf(0.1)}, {"raw_lengthscale": leaf(rng.uniform(0.4, 0.8, d)), "raw_outputscale": leaf(0.3)},
              {"raw_noise": leaf(_inv_softplus(0.05))})
    value, info = gp_util.target_logml(prior, likelihood)(X, y, seed, params_mean=params[0], params_kernel=params[1],
                                                          params_likelihood=params[2])
    value.backward()
    for group in params:
        for name, q in group.items():
            assert q.grad is not None and torch.isfinite(q.grad).all() and q.grad.abs().max() > 0, name
    # the dense expression of the value, from the same probes
    with torch.no_grad():
        raw_n = params[2]["raw_noise"]
        A = _dense_cov("matern32", X, params[1]["raw_lengthscale"], params[1]["raw_outputscale"], raw_n)
        A = A + (constrain(raw_n) - torch.nn.functional.softplus(raw_n)) * torch.eye(n, dtype=F64, device=DEV)
        resid = _np(y - params[0]["constant_value"])
        A_np = _np(A)
        if preconditioned:
            cov = RbfGramOp(X, noise_minval=1e-4, kernel="matern32").bind(params[1]["raw_lengthscale"], params[1]["raw_outputscale"], raw_n)
            pre, _ = precondition(low_rank.without_noise(cov), n)
            s = float(constrain(raw_n))
            z = _np(pre.sample(seed, p, s))
            L = _np(pre.lt).T
            M = s * np.eye(n) + L @ L.T
            logdet = np.linalg.slogdet(M)[1] + mb.dense_quadform(A_np, M, z).mean()
        else:
            z = _np(hutchinson.sampler_rademacher(torch.empty(n, dtype=F64, device=DEV), num=p)(seed))
            logdet = mb.dense_quadform(A_np, None, z).mean()
        want = -0.5 * resid @ np.linalg.solve(A_np, resid) - 0.5 * logdet - n / 2 * math.log(2 * math.pi)
    err = abs(float(value) - want) / abs(want)
    print(f"preconditioned {preconditioned}: value {float(value):.12g} dense {want:.12g} rel {err:.2e}")
    assert err <= 1e-9, (float(value), want)
    aux = info["logpdf"] if preconditioned else info
    assert aux["solve"]["residual_abs"].shape == (n,) and aux["logdet"]["depth"].shape == (p,)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    A, P, *_ = _rbf_problem(70, F64, 0)
    b = torch.ones(70, dtype=F64, device=DEV)
    sharded = RowShardedOp.__new__(RowShardedOp)  # (a real one needs a process group; the refusal does not look at it)
    solve = cg.mbcg_fixed_step(4)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        solve(sharded, b, None)
    with pytest.raises(TypeError, match="P must be None"):
        solve(A, b, lambda v: v)
    # a callable operator: forward works, backward refuses
    dense = torch.tensor(mb.table_setting()[2], device=DEV, requires_grad=True)
    z = hutchinson.sampler_rademacher(torch.empty(96, dtype=F64, device=DEV), num=2)(0)
    logpdf = gp_util.logpdf_mbcg(solve, num_probes=2)
    value, _ = logpdf(torch.ones(96, dtype=F64, device=DEV), z, mean=torch.zeros(96, dtype=F64, device=DEV),
                      cov_matvec=CallbackOp(lambda v, M: M @ v).bind(dense))
    assert torch.isfinite(value)
    with pytest.raises(NotImplementedError, match="native operators only"):
        value.backward()
    # the C-level codes, with real device pointers
    lib = _lib.get()
    desc = DenseOp().descriptor((dense.detach(),), F64, 96)
    buf = torch.zeros(4 * 96, dtype=F64, device=DEV)
    ws = _lib.scratch(int(lib.mfx_mbcg_workspace_bytes(ctypes.byref(desc), 96, 1, 0, 4)), DEV)
    ptr = _lib.ptr(buf)

    def call(maxiter=4, tdiag=ptr, ws_bytes=ws.numel(), nrows=0):
        desc.nrows = nrows
        return lib.mfx_mbcg_solve(ctypes.byref(desc), ptr, 96, 96, 1, None, 0, None, None, maxiter, 0, 1.0, 0.0, 0, ptr, ptr, ptr, ptr,
                                  tdiag, ptr, ptr, ptr, _lib.ptr(ws), ws_bytes, _lib.stream_ptr(DEV))

    assert call(maxiter=0) == -1 and call(tdiag=None) == -1 and call(nrows=64) == -2 and call(ws_bytes=256) == -4
    torch.cuda.synchronize()
    assert torch.all(buf == 0)  # nothing was launched


# ---- 9. CLI --------------------------------------------------------------------------------------------------------------------
def test_training_cli_two_epochs_on_the_protein_slice(tmp_path):
    g = np.load(os.path.join(GOLD, "uci_protein_2048.npz"))
    X = np.asarray(g["X"], dtype=np.float64)
    rng = np.random.default_rng(8)
    y = np.sin(X @ (rng.standard_normal(X.shape[1]) / 3.0)) + 0.1 * rng.standard_normal(len(X))  # the fixture holds inputs only
    folder = tmp_path / "data" / "uci" / "protein"
    os.makedirs(folder)
    with gzip.open(folder / "data.csv.gz", "wt") as f:
        np.savetxt(f, np.column_stack([X, y]), delimiter=",", header=",".join(f"c{i}" for i in range(X.shape[1] + 1)), comments="")
    r = subprocess.run([sys.executable, TRAIN, "--name", "mbcg", "--seed", "1", "--dataset", "protein", "--rank_precon", "20",
                        "--num_partitions", "1", "--num_matvecs", "30", "--num_samples", "8", "--num_epochs", "2", "--cg_tol", "1.0"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "synthetic stand-in" not in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 2
    losses = [float(ln.split("loss:")[1].split(",")[0]) for ln in lines]
    assert all(np.isfinite(losses)), losses
    assert np.isfinite(float(r.stdout.split("NLL:")[1].split()[0])) and np.isfinite(float(r.stdout.split("RMSE:")[1].split()[0]))
