"""Gradients with respect to the kernel inputs X of the Gram operator (mfx_op_grads.x, the input sweep of libmfx).

The reference is a torch-fp64 dense restatement of the three kernels of util/gp_util.py:69-184 -- the |x|^2 + |y|^2 - 2 x.y
expansion, the clamp at 0, sqrt(3) for Matern-3/2, +eps inside the square roots -- differentiated by torch autograd, with the
diagonal and exactly duplicated pairs held constant (the reference's max(0, .) passes no gradient there; autodiff through the
expansion would add rounding noise on the diagonal).  Errors are measured against the row's absolute term sum
sum_j |(S_aj + S_ja) wl_aj (xs_ac - xs_jc)| s / l_c.  Tolerances are fixed per dtype."""

import math

import pytest
import torch

from matfree_extensions import _lib, cg, hutchinson, lanczos
from matfree_extensions.operators import DenseOp, RbfGramOp
from matfree_extensions.util import gp_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {torch.float64: 1e-9, torch.float32: 1e-3}  # per element, relative to the row's absolute term sum


def inv_softplus(v):
    return math.log(math.expm1(v))


def raw_params(d, ard, dtype=torch.float64):
    ls = [inv_softplus(0.7 + 0.15 * c) for c in range(d)] if ard else inv_softplus(1.1)
    return (torch.tensor(ls, dtype=dtype, device=DEV, requires_grad=True),
            torch.tensor(inv_softplus(0.8), dtype=dtype, device=DEV, requires_grad=True),
            torch.tensor(inv_softplus(0.3), dtype=dtype, device=DEV, requires_grad=True))


def constrained(raw, noise_minval=0.0):
    sp = torch.nn.functional.softplus
    return sp(raw[0]).reshape(-1), sp(raw[1]), noise_minval + sp(raw[2])


def ref_gram(X, ls, s, kind, eps):
    """s K(X, X) in torch fp64, as util/gp_util.py:69-184 writes it, diagonal and duplicated pairs held constant."""
    xs = X / ls
    sq = (xs * xs).sum(-1)
    dist = (sq[:, None] + sq[None, :] - 2.0 * xs @ xs.T).clamp_min(0.0)
    if kind == "rbf":
        k = torch.exp(-dist / 2)
    elif kind == "matern32":
        r = torch.sqrt(3.0 * dist + eps)
        k = (1 + r) * torch.exp(-r)
    else:
        r = torch.sqrt(dist + eps)
        k = torch.exp(-r)
    same = (X[:, None, :] == X[None, :, :]).all(-1)
    return s * torch.where(same, k.detach(), k)


def term_sums(X, ls, s, kind, S, eps):
    """sum_j |(S_aj + S_ja) wl_aj (xs_ac - xs_jc)| s / l_c, column by column (n x n at a time)."""
    with torch.no_grad():
        xs = X / ls
        dist = torch.zeros((X.shape[0], X.shape[0]), dtype=X.dtype, device=X.device)
        for c in range(X.shape[1]):
            dist += (xs[:, c, None] - xs[None, :, c]) ** 2
        if kind == "rbf":
            wl = torch.exp(-dist / 2)
        elif kind == "matern32":
            wl = 3 * torch.exp(-torch.sqrt(3 * dist + eps))
        else:
            r = torch.sqrt(dist + eps)
            wl = torch.where(dist > 0, torch.exp(-r) / r, torch.zeros_like(r))
        W = (S + S.T).abs() * wl
        lsv = ls.expand(X.shape[1])
        return torch.stack([(W * (xs[:, c, None] - xs[None, :, c]).abs()).sum(1) * s / lsv[c] for c in range(X.shape[1])], 1)


# (kernel, ard, dtype, precision, d, n, batch, duplicates): every kernel meets the VALU register sweep (d <= 32), the wide sweep
# (d > 32) and the shapes where the fp32 operator runs on the matrix cores (f16x3, n >= 256, d <= 16, batch >= 16 or n >= 2048)
CASES = [
    ("rbf", True, torch.float64, "f16x3", 3, 127, 3, False),
    ("matern32", False, torch.float64, "f16x3", 40, 300, 1, False),
    ("matern12", True, torch.float64, "f16x3", 12, 300, 3, True),
    ("rbf", False, torch.float32, "fp32", 1, 5, 1, False),
    ("matern32", True, torch.float32, "f16x3-matvec", 8, 2100, 3, False),
    ("matern12", False, torch.float32, "f16x3", 16, 4099, 16, False),
    ("rbf", True, torch.float32, "f16x3", 20, 2100, 16, False),
    ("matern32", True, torch.float32, "f16x3", 40, 300, 16, True),
    ("matern12", True, torch.float64, "f16x3", 40, 127, 16, False),
    ("rbf", False, torch.float32, "f16x3", 12, 300, 16, True),
    ("matern32", False, torch.float64, "f16x3", 1, 4099, 1, False),
    ("rbf", True, torch.float64, "f16x3", 16, 2100, 16, True),
    ("matern12", True, torch.float32, "fp32", 8, 300, 16, False),
    ("matern32", True, torch.float64, "f16x3", 8, 300, 40, True),  # two batch chunks of 32, the second partial
    ("rbf", False, torch.float32, "f16x3", 40, 300, 40, False),
    ("rbf", True, torch.float64, "f16x3", 24, 300, 3, False),  # padded d = 32 in fp64
]


@pytest.mark.parametrize("kind,ard,dtype,precision,d,n,batch,dups", CASES)
def test_matvec_vjp_wrt_inputs(kind, ard, dtype, precision, d, n, batch, dups):
    g = torch.Generator(device=DEV).manual_seed(n * 31 + d)
    X0 = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32).double()  # representable in either dtype
    if dups:
        X0[1] = X0[0]
        X0[n // 2] = X0[n - 1]
    U = torch.randn(batch, n, device=DEV, generator=g, dtype=torch.float32).to(dtype)
    V = torch.randn(batch, n, device=DEV, generator=g, dtype=torch.float32).to(dtype)
    raw = raw_params(d, ard)
    X = X0.clone().requires_grad_(True)
    op = RbfGramOp(X.to(dtype), precision=precision, kernel=kind)  # the gradient comes back through .to(dtype)
    (gx,) = torch.autograd.grad((U * op(V, *raw)).sum(), X)
    assert gx.shape == X.shape and torch.isfinite(gx).all()

    eps = float(torch.finfo(dtype).eps)
    ls, s, _ = (t.detach().to(dtype).double() for t in constrained(raw))
    Xr = X0.clone().requires_grad_(True)
    S = U.double().T @ V.double()
    (gref,) = torch.autograd.grad((S * ref_gram(Xr, ls, s, kind, eps)).sum(), Xr)
    scale = term_sums(X0, ls, s, kind, S, eps)
    err = (gx - gref).abs() / (scale + 1e-300)
    assert float(err.max()) <= TOL[dtype], (float(err.max()), int(err.argmax()) // d)


def slq_dense(X, ls, s, nz, v, kind):
    A = ref_gram(X, ls, s, kind, float(torch.finfo(torch.float64).eps)) + nz * torch.eye(X.shape[0], dtype=X.dtype, device=X.device)
    lam, Q = torch.linalg.eigh(A)
    w = Q.T @ v
    return (w * w * torch.log(lam)).sum()


@pytest.mark.parametrize("reortho", ["full", "none"])
def test_slq_full_depth_matches_eigh(reortho):
    n = k = 48
    d = 3
    g = torch.Generator(device=DEV).manual_seed(5)
    X0 = torch.rand(n, d, device=DEV, generator=g, dtype=torch.float64) * 2 - 1
    v = torch.randn(n, device=DEV, generator=g, dtype=torch.float64)
    raw = raw_params(d, True)
    X = X0.clone().requires_grad_(True)
    integrand = lanczos.integrand_spd(torch.log, k, RbfGramOp(X, kernel="matern32"), reortho=reortho)
    (gx,) = torch.autograd.grad(integrand(v, *raw), X)
    Xr = X0.clone().requires_grad_(True)
    ls, s, nz = (t.detach() for t in constrained(raw))
    (gref,) = torch.autograd.grad(slq_dense(Xr, ls, s, nz, v, "matern32"), Xr)
    assert float((gx - gref).abs().max()) <= 1e-8 * float(gref.abs().max())
    # below full depth, differentiating through the loop (custom_vjp=False, the op's own matvec VJP) and the adjoint agree
    gs = []
    for custom in (True, False):
        Xc = X0.clone().requires_grad_(True)
        integ = lanczos.integrand_spd(torch.log, 12, RbfGramOp(Xc, kernel="matern32"), reortho=reortho,
                                     use_adjoints_for_tridiag=custom)
        (gc,) = torch.autograd.grad(integ(v, *raw), Xc)
        gs.append(gc)
    assert float((gs[0] - gs[1]).abs().max()) <= 1e-8 * float(gs[1].abs().max())


def dense_operator_matrix(X, raw, kind, dtype, noise_minval=0.0):
    ls, s, nz = (t.to(dtype) for t in constrained(raw, noise_minval))
    Xd = X.to(dtype)
    eps = float(torch.finfo(dtype).eps)
    return ref_gram(Xd, ls, s, kind, eps) + nz * torch.eye(X.shape[0], dtype=dtype, device=X.device)


@pytest.mark.parametrize("dtype,n,tol", [(torch.float64, 600, 1e-8), (torch.float32, 2100, 2e-3)])
def test_independent_path_through_a_dense_operator(dtype, n, tol):
    """K(X) + noise I built densely in torch, handed to DenseOp: its native adjoint and torch's chain rule give an X gradient
    that never touches the input sweep."""
    d, k, p = 3, 10, 16
    g = torch.Generator(device=DEV).manual_seed(7)
    X0 = torch.rand(n, d, device=DEV, generator=g, dtype=torch.float32).double() * 2 - 1
    V = torch.randint(0, 2, (p, n), device=DEV, generator=g).to(dtype) * 2 - 1
    raw = raw_params(d, True)
    X1 = X0.clone().requires_grad_(True)
    (g_gram,) = torch.autograd.grad(lanczos.integrand_spd(torch.log, k, RbfGramOp(X1.to(dtype), kernel="rbf"))(V, *raw).sum(), X1)
    X2 = X0.clone().requires_grad_(True)
    A = dense_operator_matrix(X2, raw, "rbf", dtype)
    (g_dense,) = torch.autograd.grad(lanczos.integrand_spd(torch.log, k, DenseOp())(V, A).sum(), X2)
    assert torch.isfinite(g_gram).all()
    assert float((g_gram - g_dense).abs().max()) <= tol * float(g_dense.abs().max())
    # the integrand that re-uses the forward basis in its backward pass (one matvec VJP): the same on both operators
    X3, X4 = X0.clone().requires_grad_(True), X0.clone().requires_grad_(True)
    reuse = lanczos.integrand_spd_custom_vjp_reuse
    (g_gram,) = torch.autograd.grad(reuse(torch.log, k, RbfGramOp(X3.to(dtype), kernel="rbf"))(V, *raw).sum(), X3)
    A = dense_operator_matrix(X4, raw, "rbf", dtype)
    (g_dense,) = torch.autograd.grad(reuse(torch.log, k, DenseOp())(V, A).sum(), X4)
    assert float((g_gram - g_dense).abs().max()) <= tol * float(g_dense.abs().max())


def test_end_to_end_log_marginal_likelihood_through_a_linear_layer():
    """target_logml(logpdf_krylov(cg_fixed_step, krylov_logdet_slq)) on inputs = Linear(features): the layer's weights get the
    gradient the dense-operator path of the previous test gives."""
    n, f, d, k, p, steps, minval = 500, 5, 3, 12, 8, 60, 1e-3
    dt = torch.float64
    gen = torch.Generator(device=DEV).manual_seed(3)
    feats = torch.rand(n, f, device=DEV, generator=gen, dtype=dt) * 2 - 1
    y = torch.sin(feats.sum(-1)) + 0.1 * torch.randn(n, device=DEV, generator=gen, dtype=dt)
    torch.manual_seed(0)
    net = torch.nn.Linear(f, d).to(device=DEV, dtype=dt)
    raw = raw_params(d, False)
    sample = hutchinson.sampler_rademacher(torch.empty(n, dtype=dt, device=DEV), num=p)
    logdet = gp_util.krylov_logdet_slq(k, sample=sample, num_batches=1)
    logpdf = gp_util.logpdf_krylov(solve=cg.cg_fixed_step(steps), logdet=logdet)
    k_fun, _ = gp_util.kernel_scaled_rbf(shape_in=(d,), shape_out=())
    m_fun, _ = gp_util.mean_constant(shape_out=())
    lik, _ = gp_util.likelihood_pdf(gp_util.gram_matvec(), logpdf, constrain=gp_util.constraint_greater_than(minval))
    loss = gp_util.target_logml(gp_util.model_gp(m_fun, k_fun), lik)
    cval = torch.tensor(0.1, dtype=dt, device=DEV)
    value, _ = loss(net(feats), y, 11, params_mean={"constant_value": cval},
                    params_kernel={"raw_lengthscale": raw[0], "raw_outputscale": raw[1]}, params_likelihood={"raw_noise": raw[2]})
    g_gram = torch.autograd.grad(value, list(net.parameters()))
    A = dense_operator_matrix(net(feats), raw, "rbf", dt, noise_minval=minval)
    value_d, _ = logpdf(y, 11, mean=cval.expand(n), cov_matvec=DenseOp().bind(A))
    g_dense = torch.autograd.grad(value_d, list(net.parameters()))
    assert abs(float(value.detach()) - float(value_d.detach())) <= 1e-8 * abs(float(value_d.detach()))
    # (a stationary kernel does not see the bias: its gradient is 0 up to round-off, so one scale for all)
    scale = max(float(b.abs().max()) for b in g_dense)
    assert scale > 0
    for a, b in zip(g_gram, g_dense):
        assert a is not None and torch.isfinite(a).all()
        assert float((a - b).abs().max()) <= 1e-7 * scale, (a, b)


def test_opt_out_is_free():
    """Hyper-parameter gradients: bitwise the same for X, X.detach() and an X that requires grad (the input sweep writes only
    `x`).  Timed scopes per class: the same in all three.  What this cannot show: mfx_timing counts class SCOPES, not kernel
    launches, so one more kernel inside the class-1 scope (the input sweep) leaves the counts unchanged; that the x == NULL path
    launches exactly the kernels it did before is checked on the code objects, not here."""
    n, d, k, p = 2100, 8, 10, 16
    g = torch.Generator(device=DEV).manual_seed(9)
    X0 = torch.randn(n, d, device=DEV, generator=g)
    V = torch.randint(0, 2, (p, n), device=DEV, generator=g).float() * 2 - 1

    def run(X):
        raw = raw_params(d, True, torch.float32)
        _lib.timing_reset()
        _lib.timing_enable(True)
        try:
            value = lanczos.integrand_spd(torch.log, k, RbfGramOp(X))(V, *raw).sum()
            grads = torch.autograd.grad(value, list(raw))
            torch.cuda.synchronize()
            launches = [_lib.timing_read(c)[1] for c in range(3)]
        finally:
            _lib.timing_enable(False)
        return grads, launches

    g_plain, l_plain = run(X0)
    g_detached, l_detached = run(X0.clone().requires_grad_(True).detach())
    g_input, l_input = run(X0.clone().requires_grad_(True))
    assert l_plain == l_detached
    for a, b, c in zip(g_plain, g_detached, g_input):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert l_input == l_plain  # (timed scopes: the input sweep runs inside the parameter sweep's class-1 scope)


def test_custom_vjp_estimator_refuses_a_closed_over_input_gradient():
    """hutchinson_custom_vjp differentiates w.r.t. its parameters only: an integrand over an operator whose X requires grad is
    refused (as jax.custom_vjp refuses closed-over tracers), not silently left without inputs.grad."""
    n, d = 300, 3
    X = torch.randn(n, d, device=DEV, dtype=torch.float64).requires_grad_(True)
    raw = raw_params(d, False)
    sample = hutchinson.sampler_rademacher(torch.empty(n, dtype=torch.float64, device=DEV), num=4)
    integrand = lanczos.integrand_spd(torch.log, 5, RbfGramOp(X))
    with pytest.raises(NotImplementedError, match="closes over"):
        hutchinson.hutchinson_custom_vjp(integrand, sample)(3, *raw)
    with torch.no_grad():  # no gradient wanted: nothing to refuse
        hutchinson.hutchinson_custom_vjp(integrand, sample)(3, *raw)
    (g,) = torch.autograd.grad(hutchinson.hutchinson_custom_vjp(lanczos.integrand_spd(torch.log, 5, RbfGramOp(X.detach())), sample)(
        3, *raw), raw[1])
    assert torch.isfinite(g)
