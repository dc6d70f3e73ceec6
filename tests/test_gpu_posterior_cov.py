"""The joint GP predictive covariance: RbfGramOp.posterior_covariance (right-hand sides K(xs_c, X) by mfx_gram_block, batched solves,
backward through mfx_gram_cross_vjp_dense and mfx_op_vjp_params), likelihood_condition_cov[_p] and posterior_samples.

The reference is the dense torch-fp64 expression Kss - Ksx A^-1 Kxs (torch.linalg.solve) on the Gram operator's formulas --
the |x|^2 + |y|^2 - 2 x.y expansion clamped at 0, eps of the compute dtype inside Matern's square root, exactly duplicated pairs
(the diagonal of Kss among them) at distance 0 and held constant -- differentiated by torch autograd.  n = 300, m = 37.

Tolerances are those of the same quantities in tests/test_gpu_posterior_var.py: a covariance entry against s like a variance
(VAR_TOL), a gradient against the largest entry of its reference (GRAD_TOL, floored at s), chunking at 1e-10 of the largest entry."""

import functools
import math

import pytest
import torch

from matfree_extensions import cg, hutchinson, low_rank
from matfree_extensions.operators import RbfGramOp
from matfree_extensions.util import gp_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VAR_TOL = {torch.float64: 1e-9, torch.float32: 1e-3}  # |cov - ref| / s             (test_gpu_posterior_var.py: VAR_TOL)
GRAD_TOL = {torch.float64: 1e-7, torch.float32: 5e-3}  # |g - ref| / max(max |ref|, s) (test_gpu_posterior_var.py: GRAD_TOL)
N, M = 300, 37
OPERATORS = [("rbf", False, 3), ("matern52", True, 5)]
NAMES = ("xs", "raw_l", "raw_s", "raw_noise", "X")


def inv_softplus(v):
    return math.log(math.expm1(v))


def solver(dtype):
    if dtype == torch.float64:
        return cg.cg_adaptive(atol=1e-12, rtol=0.0, maxiter=2000, miniter=1)  # run to convergence
    return cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=1000, miniter=1)


def raw_params(d, ard):
    ls = [inv_softplus(0.7 + 0.15 * c) for c in range(d)] if ard else inv_softplus(1.1)
    return tuple(torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True)
                 for v in (ls, inv_softplus(0.8), inv_softplus(0.5)))


def kfun(dist, kind, eps):
    if kind == "rbf":
        return torch.exp(-dist / 2)
    r = torch.sqrt(5.0 * dist + eps)
    return (1 + r + r * r / 3) * torch.exp(-r)


def ref_cross(Xa, Xb, ls, s, kind, eps):
    xa, xb = Xa / ls, Xb / ls
    dist = ((xa * xa).sum(-1)[:, None] + (xb * xb).sum(-1)[None, :] - 2.0 * xa @ xb.T).clamp_min(0.0)
    same = (Xa[:, None, :] == Xb[None, :, :]).all(-1)
    k = kfun(torch.where(same, torch.zeros_like(dist), dist), kind, eps)
    return s * torch.where(same, k.detach(), k)


def ref_cov(xs, X, ls, s, nz, kind, eps):
    A = ref_cross(X, X, ls, s, kind, eps) + nz * torch.eye(X.shape[0], dtype=torch.float64, device=DEV)
    Ksx = ref_cross(xs, X, ls, s, kind, eps)
    return ref_cross(xs, xs, ls, s, kind, eps) - Ksx @ torch.linalg.solve(A, Ksx.T)


@functools.lru_cache(maxsize=None)
def problem(kind, ard, d):
    g = torch.Generator(device=DEV).manual_seed(11 + d)
    X0 = torch.randn(N, d, device=DEV, generator=g, dtype=torch.float32).double()  # representable in either dtype
    xs0 = torch.randn(M, d, device=DEV, generator=g, dtype=torch.float32).double()
    xs0[0] = X0[3]  # a test point exactly on a training point
    G = torch.randn(M, M, device=DEV, generator=g, dtype=torch.float32).double()  # not symmetric
    return X0, xs0, G


@functools.lru_cache(maxsize=None)
def reference(kind, ard, d, dtype):
    """(Sigma, gradients of sum(Sigma G) in NAMES order, s) of the dense fp64 expression, with the eps of `dtype`; computed once"""
    X0, xs0, G = problem(kind, ard, d)
    sp = torch.nn.functional.softplus
    rr = [r.detach().clone().requires_grad_(True) for r in raw_params(d, ard)]
    Xr, xsr = X0.clone().requires_grad_(True), xs0.clone().requires_grad_(True)
    cov = ref_cov(xsr, Xr, sp(rr[0]), sp(rr[1]), sp(rr[2]), kind, float(torch.finfo(dtype).eps))
    grads = torch.autograd.grad((cov * G).sum(), (xsr, *rr, Xr))
    return cov.detach(), tuple(g.detach() for g in grads), float(sp(rr[1].detach()))


def run(kind, ard, d, dtype, chunk, solve=None):
    X0, xs0, G = problem(kind, ard, d)
    raw = raw_params(d, ard)
    X, xs = X0.clone().requires_grad_(True), xs0.clone().requires_grad_(True)
    cov = RbfGramOp(X.to(dtype), kernel=kind).posterior_covariance(xs, solve or solver(dtype), *raw, chunk=chunk)
    grads = torch.autograd.grad((cov * G.to(dtype)).sum(), (xs, *raw, X))
    return cov.detach(), grads


def rel_err(got, want, floor):
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), floor)


@pytest.mark.parametrize("chunk", [64, 16, 1])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,ard,d", OPERATORS)
def test_covariance_and_gradients_match_the_dense_fp64_expression(kind, ard, d, dtype, chunk):
    cov, grads = run(kind, ard, d, dtype, chunk)
    want_cov, want, s = reference(kind, ard, d, dtype)
    assert cov.shape == (M, M) and cov.dtype == dtype
    assert torch.equal(cov, cov.T)  # bitwise
    err = float((cov.double() - want_cov).abs().max()) / s
    print(f"{kind} {dtype} chunk {chunk}: cov {err:.3e} (tol {VAR_TOL[dtype]:.0e})")
    assert err <= VAR_TOL[dtype]
    for name, gg, ww in zip(NAMES, grads, want):
        e = rel_err(gg, ww, s)
        print(f"  {name}: {e:.3e} (tol {GRAD_TOL[dtype]:.0e})")
        assert e <= GRAD_TOL[dtype], (name, e)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,ard,d", OPERATORS)
def test_diagonal_is_the_posterior_variance(kind, ard, d, dtype):
    X0, xs0, _ = problem(kind, ard, d)
    raw = raw_params(d, ard)
    op = RbfGramOp(X0.to(dtype), kernel=kind)
    with torch.no_grad():
        cov = op.posterior_covariance(xs0, solver(dtype), *raw)
        var = op.posterior_variance(xs0, solver(dtype), *raw)
    s = float(torch.nn.functional.softplus(raw[1].detach()))
    err = float((cov.diagonal() - var).abs().max()) / s
    print(f"{kind} {dtype}: diag - var {err:.3e}")
    assert err <= VAR_TOL[dtype]


@pytest.mark.parametrize("kind,ard,d", OPERATORS)
def test_chunk_size_does_not_change_the_result(kind, ard, d):
    res = [run(kind, ard, d, torch.float64, chunk) for chunk in (64, 16, 1)]
    for cov, grads in res[1:]:
        for a, b in zip((res[0][0], *res[0][1]), (cov, *grads)):
            assert torch.allclose(a, b, rtol=0, atol=1e-10 * float(a.abs().max())), float((a - b).abs().max())


def test_result_and_gradients_are_bitwise_reproducible():
    a, b = (run("matern52", True, 5, torch.float32, 16) for _ in range(2))
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


def test_only_the_requested_gradients_are_computed():
    kind, ard, d = OPERATORS[1]
    X0, xs0, G = problem(kind, ard, d)
    want = reference(kind, ard, d, torch.float64)[1]
    for pick in (3, 0):  # raw_noise alone (no cross sweep, no Kss sweep); xs alone (no Gram parameter sweep)
        raw = [r.detach() for r in raw_params(d, ard)]
        xs = xs0.clone()
        leaves = [xs, *raw]
        leaves[pick].requires_grad_(True)
        cov = RbfGramOp(X0, kernel=kind).posterior_covariance(xs, solver(torch.float64), *raw)
        (cov * G).sum().backward()
        for i, t in enumerate(leaves):
            assert (t.grad is None) == (i != pick), (pick, i)
        assert rel_err(leaves[pick].grad, want[pick], 0.0) <= GRAD_TOL[torch.float64]


def test_no_gradient_requested_keeps_the_forward():
    kind, ard, d = OPERATORS[0]
    X0, xs0, _ = problem(kind, ard, d)
    raw = [r.detach() for r in raw_params(d, ard)]
    cov, info = RbfGramOp(X0, kernel=kind).posterior_covariance(xs0, solver(torch.float64), *raw, chunk=16, return_info=True)
    assert not cov.requires_grad
    assert float((cov - reference(kind, ard, d, torch.float64)[0]).abs().max()) <= VAR_TOL[torch.float64] * reference(kind, ard, d, torch.float64)[2]
    assert info["solve"]["num_steps"].shape == (M,)  # one entry per test point, in test-point order
    assert info["solve"]["residual_abs"].shape == (M, N)


def test_gradcheck_fp64():
    g = torch.Generator(device=DEV).manual_seed(3)
    X = torch.randn(30, 2, device=DEV, generator=g, dtype=torch.float64).requires_grad_(True)
    xs = torch.randn(5, 2, device=DEV, generator=g, dtype=torch.float64).requires_grad_(True)
    rl = torch.tensor([0.2, -0.3], dtype=torch.float64, device=DEV, requires_grad=True)
    rs = torch.tensor(0.4, dtype=torch.float64, device=DEV, requires_grad=True)
    rn = torch.tensor(-1.0, dtype=torch.float64, device=DEV, requires_grad=True)
    solve = cg.cg_adaptive(atol=1e-14, rtol=0.0, maxiter=500, miniter=1)

    def f(xs, rl, rs, rn, X):
        return RbfGramOp(X, kernel="matern52").posterior_covariance(xs, solve, rl, rs, rn, chunk=2)

    assert torch.autograd.gradcheck(f, (xs, rl, rs, rn, X), eps=1e-6, atol=1e-6, rtol=1e-4)


# ---- likelihood_condition_cov[_p] and posterior_samples --------------------------------------------------------------------------

def _posterior(precond, what, observation_noise=False):
    n, m, d = 160, 23, 3
    g = torch.Generator(device=DEV).manual_seed(17)
    X = torch.rand(n, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2
    xs = torch.rand(m, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2
    xs[2] = X[7]
    y = torch.sin(X.sum(-1))
    params = dict(c=0.3, rl=[0.1, 0.3, -0.2], rs=0.3, rn=-1.0)
    p = {k: torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True) for k, v in params.items()}
    k_fun, _ = gp_util.kernel_scaled_matern_52(shape_in=(d,), shape_out=())
    m_fun, _ = gp_util.mean_constant(shape_out=())
    kw = dict(constrain=gp_util.constraint_greater_than(1e-2))
    if what == "cov":
        kw.update(observation_noise=observation_noise, chunk=8)
    if precond:
        make = gp_util.likelihood_condition_cov_p if what == "cov" else gp_util.likelihood_condition_p
        lik, _ = make(gp_util.gram_matvec(), cg.pcg_adaptive(atol=1e-12, rtol=0.0, maxiter=1000, miniter=1),
                      precondition=low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20)), **kw)
    else:
        make = gp_util.likelihood_condition_cov if what == "cov" else gp_util.likelihood_condition
        lik, _ = make(gp_util.gram_matvec(), cg.cg_adaptive(atol=1e-12, rtol=0.0, maxiter=1000, miniter=1), **kw)
    post, _ = gp_util.target_posterior(gp_util.model_gp(m_fun, k_fun), lik)(
        X, y, params_mean={"constant_value": p["c"]}, params_kernel={"raw_lengthscale": p["rl"], "raw_outputscale": p["rs"]},
        params_likelihood={"raw_noise": p["rn"]})
    out, info = post(xs)
    return X, xs, p, out, info


@pytest.mark.parametrize("precond", [False, True], ids=["cg", "pcg"])
def test_likelihood_condition_cov(precond):
    X, xs, p, (mu, cov), info = _posterior(precond, "cov")
    _, _, _, mu_plain, _ = _posterior(precond, "mean")
    assert torch.equal(mu.detach(), mu_plain.detach())  # the mean is likelihood_condition[_p]'s, bitwise
    assert info["covariance_solve"]["num_steps"].shape == (xs.shape[0],)
    assert int(info["covariance_solve"]["num_steps"].max()) < 1000
    sp = torch.nn.functional.softplus
    ls, s, nz = sp(p["rl"]), sp(p["rs"]), 1e-2 + sp(p["rn"])
    want = ref_cov(xs, X, ls, s, nz, "matern52", float(torch.finfo(torch.float64).eps))
    assert float((cov - want).abs().max()) <= VAR_TOL[torch.float64] * float(s)
    assert torch.equal(cov, cov.T)
    # observation noise: on the diagonal only, and the noise then gets its gradient through that term too
    _, _, q, (mu_o, cov_o), _ = _posterior(precond, "cov", observation_noise=True)
    assert torch.equal(mu_o.detach(), mu.detach())
    off = ~torch.eye(xs.shape[0], dtype=torch.bool, device=DEV)
    assert torch.equal(cov_o.detach()[off], cov.detach()[off])
    assert float((cov_o.diagonal() - cov.diagonal() - nz).abs().max()) <= 1e-12
    wts = torch.linspace(0.5, 2.0, xs.shape[0], dtype=torch.float64, device=DEV)
    (g_lat,) = torch.autograd.grad((wts * cov.diagonal()).sum(), (p["rn"],))
    (g_obs,) = torch.autograd.grad((wts * cov_o.diagonal()).sum(), (q["rn"],))
    assert abs(float(g_obs - g_lat) - float(wts.sum() * torch.sigmoid(p["rn"]))) <= 1e-9


def test_posterior_samples():
    X, xs, p, (mu, cov), _ = _posterior(False, "cov")
    mean, cov = mu.detach(), cov.detach()
    m, num, jitter = mean.shape[0], 5, 1e-8
    draws = gp_util.posterior_samples(1234, mean, cov, num=num, jitter=jitter)
    assert draws.shape == (num, m) and draws.dtype == mean.dtype
    assert torch.equal(draws, gp_util.posterior_samples(1234, mean, cov, num=num, jitter=jitter))  # the same key, the same draw
    assert not torch.equal(draws, gp_util.posterior_samples(1235, mean, cov, num=num, jitter=jitter))
    eps = hutchinson.sampler_normal(mean, num=num)(1234)
    target = cov + jitter * torch.eye(m, dtype=torch.float64, device=DEV)
    L = torch.linalg.cholesky(target)
    assert float((draws - (mean + eps @ L.T)).abs().max()) <= 1e-10
    assert float((L @ L.T - target).abs().max()) <= 1e-10
    # fp32 inputs: factored in fp64, cast back
    d32 = gp_util.posterior_samples(1234, mean.float(), cov.float(), num=num, jitter=1e-4)
    assert d32.dtype == torch.float32 and torch.isfinite(d32).all()
    # differentiable through torch
    mg, cg_ = mean.clone().requires_grad_(True), cov.clone().requires_grad_(True)
    gm, gc = torch.autograd.grad(gp_util.posterior_samples(1234, mg, cg_, num=num, jitter=jitter).sum(), (mg, cg_))
    assert torch.equal(gm, torch.full_like(gm, num)) and torch.isfinite(gc).all() and float(gc.abs().max()) > 0


def test_posterior_samples_refuses_an_indefinite_covariance():
    cov = torch.eye(6, dtype=torch.float64, device=DEV)
    cov[2, 2] = -0.5
    mean = torch.zeros(6, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="jitter"):
        gp_util.posterior_samples(7, mean, cov, num=3)
    assert gp_util.posterior_samples(7, mean, cov, num=3, jitter=1.0).shape == (3, 6)
