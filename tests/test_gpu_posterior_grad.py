"""Gradients of the GP posterior mean: the reverse mode of the cross-covariance matvec y = K(X_new, X) v
(RbfGramOp.cross_apply -> mfx_gram_cross_apply_t and mfx_gram_cross_vjp) and, through it, of likelihood_condition[_p].

The reference is a torch-fp64 dense restatement of s k(X_new, X) as util/gp_util.py:69-184 writes it (the |x|^2 + |y|^2 - 2 x.y
expansion, the clamp at 0, sqrt(3) for Matern-3/2, +eps inside the square roots), differentiated by torch autograd, with exactly
duplicated pairs held constant (the reference's max(0, .) passes no gradient there).  Errors are measured per element against
the absolute sum of the terms that make up that element; for the input gradients the difference xs_ac - xs_jc counts as its two
terms, because the scaled points x / l are rounded to the operator's dtype before they are subtracted (an element with a single
pair, m = 1, at a near-tie coordinate is otherwise all cancellation: 1.5e-3 in fp32 measured against |xs_ac - xs_jc|).
Tolerances are fixed per dtype."""

import math

import pytest
import torch

from matfree_extensions import cg, low_rank
from matfree_extensions.operators import RbfGramOp
from matfree_extensions.util import gp_util, pde_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {torch.float64: 1e-9, torch.float32: 1e-3}


def inv_softplus(v):
    return math.log(math.expm1(v))


def raw_params(d, ard, dtype=torch.float64):
    ls = [inv_softplus(0.7 + 0.15 * c) for c in range(d)] if ard else inv_softplus(1.1)
    return (torch.tensor(ls, dtype=dtype, device=DEV, requires_grad=True),
            torch.tensor(inv_softplus(0.8), dtype=dtype, device=DEV, requires_grad=True),
            torch.tensor(inv_softplus(0.3), dtype=dtype, device=DEV, requires_grad=True))


def kfun(dist, kind, eps):
    if kind == "rbf":
        return torch.exp(-dist / 2)
    if kind == "matern32":
        r = torch.sqrt(3.0 * dist + eps)
        return (1 + r) * torch.exp(-r)
    return torch.exp(-torch.sqrt(dist + eps))


def ref_cross(Xn, X, ls, s, kind, eps):
    """s K(Xn, X) in torch fp64, exactly duplicated pairs held constant."""
    xa, xb = Xn / ls, X / ls
    dist = ((xa * xa).sum(-1)[:, None] + (xb * xb).sum(-1)[None, :] - 2.0 * xa @ xb.T).clamp_min(0.0)
    k = kfun(dist, kind, eps)
    same = (Xn[:, None, :] == X[None, :, :]).all(-1)
    return s * torch.where(same, k.detach(), k)


def term_sums(Xn, X, ls, s, kind, S, Ybar, V, eps):
    """Absolute term sums of every gradient element: (v, xnew, X, lengthscale per dim, outputscale)."""
    with torch.no_grad():
        xa, xb = Xn / ls, X / ls
        diff = xa[:, None, :] - xb[None, :, :]  # (m, n, d)
        dist = (diff * diff).sum(-1)
        k = kfun(dist, kind, eps)
        if kind == "rbf":
            wl = k
        elif kind == "matern32":
            wl = 3 * torch.exp(-torch.sqrt(3 * dist + eps))
        else:
            r = torch.sqrt(dist + eps)
            wl = torch.where(dist > 0, torch.exp(-r) / r, torch.zeros_like(r))
        lsv = ls.expand(X.shape[1])
        W = S.abs() * wl  # (m, n)
        t_v = s * (k.T[None] * Ybar.abs()[:, None, :]).sum(-1)  # (p, n): sum_a |K_aj ybar_b[a]|
        mag = xa.abs()[:, None, :] + xb.abs()[None, :, :]  # |xs_ac| + |xs_jc|: the two terms of (xs_ac - xs_jc)
        t_xn = (W[:, :, None] * mag).sum(1) * s / lsv
        t_x = (W[:, :, None] * mag).sum(0) * s / lsv
        t_ls = (W[:, :, None] * diff * diff).sum((0, 1)) * s / lsv
        t_s = (S.abs() * k).sum()
        return t_v, t_xn, t_x, t_ls, t_s


def check(got, want, scale, tol, what):
    err = (got - want).abs() / (scale + 1e-300)
    assert float(err.max()) <= tol, (what, float(err.max()))


# (kernel, ard, dtype, d, m, n, p, duplicates): every kernel, both lengthscale forms and dtypes, d in {1, 3, 8, 11, 16, 17, 40} -- the
# register sweeps with the shared and the separate lengthscale / input forms (padded d <= 16 and 32) and the wide sweep
CASES = [
    ("rbf", True, torch.float64, 3, 70, 700, 3, True),
    ("matern32", False, torch.float64, 1, 333, 2049, 1, False),
    ("matern12", True, torch.float64, 8, 1, 700, 9, False),
    ("rbf", False, torch.float64, 17, 70, 2049, 3, True),
    ("matern32", True, torch.float64, 17, 333, 700, 9, False),
    ("matern32", True, torch.float64, 40, 70, 700, 3, True),
    ("matern12", False, torch.float64, 40, 333, 700, 1, False),
    ("rbf", True, torch.float32, 8, 333, 2049, 9, True),
    ("matern32", True, torch.float32, 17, 1, 2049, 1, False),
    ("matern12", False, torch.float32, 3, 70, 700, 3, True),
    ("rbf", False, torch.float32, 40, 70, 700, 9, False),
    ("matern12", True, torch.float32, 40, 333, 2049, 3, True),
    ("matern32", False, torch.float32, 1, 70, 700, 9, True),
    ("rbf", True, torch.float32, 17, 70, 700, 1, False),
    ("matern32", True, torch.float64, 11, 70, 300, 2, True),  # padded d = 12 and 16
    ("rbf", False, torch.float64, 16, 70, 300, 5, False),
    ("rbf", True, torch.float32, 11, 70, 300, 5, True),
    ("matern32", False, torch.float32, 16, 70, 300, 2, False),
]


def _problem(d, m, n, p, dups, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    X0 = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32).double()  # representable in either dtype
    Xn0 = torch.randn(m, d, device=DEV, generator=g, dtype=torch.float32).double()
    if dups:
        Xn0[0] = X0[3]
        if m > 2:
            Xn0[m - 1] = X0[n - 1]
    V = torch.randn(p, n, device=DEV, generator=g, dtype=torch.float32).double()
    Ybar = torch.randn(p, m, device=DEV, generator=g, dtype=torch.float32).double()
    return X0, Xn0, V, Ybar


@pytest.mark.parametrize("kind,ard,dtype,d,m,n,p,dups", CASES)
def test_cross_vjp_matches_fp64_autograd(kind, ard, dtype, d, m, n, p, dups):
    X0, Xn0, V0, Ybar = _problem(d, m, n, p, dups, dtype, seed=m * 7 + n + d)
    raw = raw_params(d, ard)
    X = X0.clone().requires_grad_(True)
    Xn = Xn0.clone().requires_grad_(True)
    V = V0.to(dtype).requires_grad_(True)
    op = RbfGramOp(X.to(dtype), kernel=kind)
    y = op.cross_apply(Xn, V, *raw)  # xnew.to(dtype) and X.to(dtype) pass the gradient back
    assert y.shape == (p, m) and y.dtype == dtype
    gv, gxn, gx, gl, gs, gn = torch.autograd.grad((Ybar.to(dtype) * y).sum(), (V, Xn, X, *raw), allow_unused=True)
    assert gn is None  # no noise in the cross-covariance

    eps = float(torch.finfo(dtype).eps)
    sp = torch.nn.functional.softplus
    ls = sp(raw[0]).detach().to(dtype).double().reshape(-1).requires_grad_(True)
    s = sp(raw[1]).detach().to(dtype).double().requires_grad_(True)
    Xr, Xnr, Vr = X0.clone().requires_grad_(True), Xn0.clone().requires_grad_(True), V0.clone().requires_grad_(True)
    K = ref_cross(Xnr, Xr, ls, s, kind, eps)
    rv, rxn, rx, rl, rs = torch.autograd.grad((Ybar * (Vr @ K.T)).sum(), (Vr, Xnr, Xr, ls, s))
    S = Ybar.T @ V0
    t_v, t_xn, t_x, t_ls, t_s = term_sums(Xn0, X0, ls.detach(), s.detach(), kind, S, Ybar, V0, eps)
    sig_l, sig_s = torch.sigmoid(raw[0].detach()).reshape(-1), torch.sigmoid(raw[1].detach())
    tol = TOL[dtype]
    check(gv.double(), rv, t_v, tol, "v")
    check(gxn, rxn, t_xn, tol, "xnew")
    check(gx, rx, t_x, tol, "X")
    check(gl.reshape(-1), rl * sig_l, (t_ls if ard else t_ls.sum()) * sig_l, tol, "lengthscale")
    check(gs, rs * sig_s, t_s * sig_s, tol, "outputscale")


# The VALU matvec picks its kernel from the padded dimension (d = 3, 8, 11, 16, 24 pad to 4, 8, 12, 16, 32; 40 is wide) and the
# vectors per workgroup from p (1, 2, 3, 9 -> 1, 2, 4, 8, the last two with a ragged last chunk; wide: 1, 4 and, in fp32 only, 8):
# every pair in both dtypes, forward (rows X_new, columns X) and transposed (rows X, columns X_new); m != n, neither a tile multiple
MATVEC = [(dtype, d, p) for dtype in (torch.float64, torch.float32) for d in (3, 8, 11, 16, 24, 40) for p in (1, 2, 3, 9)
          if d < 40 or p in (1, 3) or (p == 9 and dtype == torch.float32)]


@pytest.mark.parametrize("dtype,d,p", MATVEC, ids=[f"{'fp64' if t == torch.float64 else 'fp32'}-d{d}-p{p}" for t, d, p in MATVEC])
def test_cross_matvec_and_its_transpose_at_every_padded_dimension_and_vector_count(dtype, d, p):
    kind, m, n = ("rbf", "matern32")[(d + p) % 2], 70, 300
    X0, Xn0, V0, Ybar = _problem(d, m, n, p, True, dtype, seed=10 * d + p)
    raw = raw_params(d, True)
    V = V0.to(dtype).requires_grad_(True)
    y = RbfGramOp(X0.to(dtype), kernel=kind).cross_apply(Xn0, V, *raw)
    (gv,) = torch.autograd.grad((Ybar.to(dtype) * y).sum(), V)  # K(X, X_new) ybar: mfx_gram_cross_apply_t
    assert y.shape == (p, m) and gv.shape == (p, n)
    with torch.no_grad():
        sp = torch.nn.functional.softplus
        ls, s = sp(raw[0]).to(dtype).double().reshape(-1), sp(raw[1]).to(dtype).double()
        K = ref_cross(Xn0, X0, ls, s, kind, float(torch.finfo(dtype).eps))  # (m, n), every entry positive
        check(y.double(), V0 @ K.T, V0.abs() @ K.T, TOL[dtype], "y")
        check(gv.double(), Ybar @ K, Ybar.abs() @ K, TOL[dtype], "v")


@pytest.mark.parametrize("d", [3, 40])
def test_partial_requests_agree_with_the_full_request(d):
    """The backward skips what needs_input_grad does not ask for; every subset gives what the full request gives (fp64).  The
    lengthscale sums move between the X_new and the X sweep with the request, so they agree to rounding, not bitwise."""
    X0, Xn0, V0, Ybar = _problem(d, 33, 517, 2, True, torch.float64, seed=11)
    raw = raw_params(d, True)
    X, Xn, V = (t.clone().requires_grad_(True) for t in (X0, Xn0, V0))
    full = torch.autograd.grad((Ybar * RbfGramOp(X, kernel="matern32").cross_apply(Xn, V, *raw)).sum(), (V, Xn, X, raw[0], raw[1]))
    for pick in ([0], [1], [2], [3, 4], [1, 3], [2, 3, 4], [0, 2]):
        leaves = [t.detach().clone().requires_grad_(i in pick) for i, t in enumerate((V0, Xn0, X0, raw[0], raw[1]))]
        V, Xn, X, rl, rs = leaves
        y = RbfGramOp(X, kernel="matern32").cross_apply(Xn, V, rl, rs, raw[2].detach())
        got = torch.autograd.grad((Ybar * y).sum(), [leaves[i] for i in pick])
        for i, gv in zip(pick, got):
            assert torch.allclose(gv, full[i], rtol=1e-12, atol=1e-12 * float(full[i].abs().max())), (pick, i)


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
def test_gradcheck_fp64(kind):
    g = torch.Generator(device=DEV).manual_seed(3)
    X = torch.randn(40, 2, device=DEV, generator=g, dtype=torch.float64).requires_grad_(True)
    xn = torch.randn(7, 2, device=DEV, generator=g, dtype=torch.float64).requires_grad_(True)
    v = torch.randn(2, 40, device=DEV, generator=g, dtype=torch.float64).requires_grad_(True)
    rl = torch.tensor([0.2, -0.3], dtype=torch.float64, device=DEV, requires_grad=True)
    rs = torch.tensor(0.4, dtype=torch.float64, device=DEV, requires_grad=True)
    rn = torch.tensor(-1.0, dtype=torch.float64, device=DEV)

    def f(v, xn, rl, rs, X):
        return RbfGramOp(X, kernel=kind).cross_apply(xn, v, rl, rs, rn)

    assert torch.autograd.gradcheck(f, (v, xn, rl, rs, X), eps=1e-6, atol=1e-6, rtol=1e-4)


def _posterior_case(precond):
    n, m, d = 160, 23, 3
    g = torch.Generator(device=DEV).manual_seed(17)
    X = (torch.rand(n, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2).requires_grad_(True)
    xs = (torch.rand(m, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2).requires_grad_(True)
    y = torch.sin(X.detach().sum(-1)).requires_grad_(True)
    c = torch.tensor(0.3, dtype=torch.float64, device=DEV, requires_grad=True)
    rl = torch.tensor([0.1, 0.3, -0.2], dtype=torch.float64, device=DEV, requires_grad=True)
    rs = torch.tensor(0.3, dtype=torch.float64, device=DEV, requires_grad=True)
    rn = torch.tensor(-1.0, dtype=torch.float64, device=DEV, requires_grad=True)
    k_fun, _ = gp_util.kernel_scaled_matern_32(shape_in=(d,), shape_out=())
    m_fun, _ = gp_util.mean_constant(shape_out=())
    constrain = gp_util.constraint_greater_than(1e-2)
    if precond:
        lik, _ = gp_util.likelihood_condition_p(gp_util.gram_matvec(), cg.pcg_adaptive(atol=1e-12, rtol=0.0, maxiter=1000, miniter=1),
                                                precondition=low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20)),
                                                constrain=constrain)
    else:
        lik, _ = gp_util.likelihood_condition(gp_util.gram_matvec(), cg.cg_adaptive(atol=1e-12, rtol=0.0, maxiter=1000, miniter=1),
                                              constrain=constrain)
    post, _ = gp_util.target_posterior(gp_util.model_gp(m_fun, k_fun), lik)(
        X, y, params_mean={"constant_value": c}, params_kernel={"raw_lengthscale": rl, "raw_outputscale": rs},
        params_likelihood={"raw_noise": rn})
    mu, info = post(xs)

    sp = torch.nn.functional.softplus
    eps = float(torch.finfo(torch.float64).eps)
    ls, s, nz = sp(rl), sp(rs), 1e-2 + sp(rn)
    K = ref_cross(X, X, ls, s, "matern32", eps) + nz * torch.eye(n, dtype=torch.float64, device=DEV)
    w = torch.cholesky_solve((y - c)[:, None], torch.linalg.cholesky(K))[:, 0]
    mu_ref = c + ref_cross(xs, X, ls, s, "matern32", eps) @ w
    return (X, xs, y, c, rl, rs, rn), mu, mu_ref, info


@pytest.mark.parametrize("precond", [False, True])
def test_posterior_mean_gradients_match_dense_cholesky(precond):
    inputs, mu, mu_ref, info = _posterior_case(precond)
    assert int(info["solve"]["num_steps"]) < 1000
    assert torch.allclose(mu, mu_ref, rtol=0, atol=1e-8 * float(mu_ref.abs().max()))
    targets = torch.linspace(-1.0, 1.0, mu.shape[0], dtype=torch.float64, device=DEV)
    weights = torch.linspace(0.5, 2.0, mu.shape[0], dtype=torch.float64, device=DEV)
    for loss in (lambda u: u.sum(), lambda u: pde_util.loss_mse()(weights * u, targets=targets)):
        got = torch.autograd.grad(loss(mu), inputs, retain_graph=True)
        want = torch.autograd.grad(loss(mu_ref), inputs, retain_graph=True)
        for name, gg, ww in zip(("X", "xs", "y", "constant", "raw_l", "raw_s", "raw_noise"), got, want):
            assert gg is not None, name
            assert torch.allclose(gg, ww, rtol=0, atol=1e-6 * float(ww.abs().max())), (name, float((gg - ww).abs().max()))


def test_large_n_few_test_points_fp32_is_accurate_and_reproducible():
    """n = 131072, m = 16, d = 8 (the acquisition-optimisation shape): the column split carries the X_new gradient.  Checked
    against fp64 in column chunks; two runs agree bitwise (no atomics)."""
    n, m, d = 131072, 16, 8
    g = torch.Generator(device=DEV).manual_seed(23)
    X = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32)
    xn0 = torch.randn(m, d, device=DEV, generator=g, dtype=torch.float32)
    v = torch.randn(n, device=DEV, generator=g, dtype=torch.float32)
    ybar = torch.randn(m, device=DEV, generator=g, dtype=torch.float32)
    raw = [torch.tensor(r, dtype=torch.float32, device=DEV, requires_grad=True)
           for r in ([inv_softplus(0.8 + 0.1 * c) for c in range(d)], inv_softplus(1.2), 0.0)]

    def run():
        xn = xn0.clone().requires_grad_(True)
        mu = RbfGramOp(X).cross_apply(xn, v, *raw)
        return torch.autograd.grad((ybar * mu).sum(), (xn, raw[0], raw[1]))

    a, b = run(), run()
    for ga, gb in zip(a, b):
        assert torch.equal(ga, gb)
    ls = torch.nn.functional.softplus(raw[0]).detach().double()
    s = float(torch.nn.functional.softplus(raw[1]).detach().double())
    xa = xn0.double() / ls
    ref = torch.zeros(m, d, dtype=torch.float64, device=DEV)
    scale = torch.zeros(m, d, dtype=torch.float64, device=DEV)
    for j0 in range(0, n, 16384):
        xb = X[j0:j0 + 16384].double() / ls
        diff = xa[:, None, :] - xb[None, :, :]
        k = torch.exp(-(diff * diff).sum(-1) / 2)
        S = ybar.double()[:, None] * v[j0:j0 + 16384].double()[None, :]
        ref += -(s / ls) * ((S * k)[:, :, None] * diff).sum(1)
        scale += (s / ls) * ((S.abs() * k)[:, :, None] * (xa.abs()[:, None, :] + xb.abs()[None, :, :])).sum(1)
    check(a[0].double(), ref, scale, TOL[torch.float32], "xnew")


@pytest.mark.parametrize("dtype,d", [(torch.float32, 8), (torch.float64, 40)])
def test_forward_is_bitwise_unchanged_by_requires_grad(dtype, d):
    g = torch.Generator(device=DEV).manual_seed(5)
    X = torch.randn(900, d, device=DEV, generator=g, dtype=dtype)
    xn = torch.randn(50, d, device=DEV, generator=g, dtype=dtype)
    V = torch.randn(3, 900, device=DEV, generator=g, dtype=dtype)
    raw = raw_params(d, True, dtype)
    with torch.no_grad():
        plain = RbfGramOp(X, kernel="matern12").cross_apply(xn, V, *raw)
    Xg, xg, Vg = (t.clone().requires_grad_(True) for t in (X, xn, V))
    tracked = RbfGramOp(Xg, kernel="matern12").cross_apply(xg, Vg, *raw)
    assert tracked.requires_grad and torch.equal(tracked.detach(), plain)
    one = RbfGramOp(X, kernel="matern12").cross_apply(xn, V[1], *raw)
    assert one.shape == (50,) and torch.equal(one.detach(), plain[1])
