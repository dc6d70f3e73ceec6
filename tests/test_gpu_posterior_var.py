"""The GP predictive variance: RbfGramOp.posterior_variance (batched solves against K(X, xs), backward through
mfx_gram_cross_vjp_dense and mfx_op_vjp_params) and likelihood_condition_var[_p].

The reference is a torch-fp64 dense restatement -- s k(., .) as util/gp_util.py:69-184 writes it (the |x|^2 + |y|^2 - 2 x.y
expansion, the clamp at 0, sqrt(3) for Matern-3/2, +eps inside the square roots, exactly duplicated pairs held constant), a
Cholesky factor of K + noise I, and var_a = s kappa(0) - |L^-1 K(X, xs_a)|^2 -- differentiated by torch autograd.  Errors of the
variance are measured against s; a gradient's errors against the largest term of its reference, and of the sweep oracle against
its own largest element.  Tolerances are fixed per dtype."""

import ctypes as C
import math

import pytest
import torch

from matfree_extensions import _lib, cg, low_rank
from matfree_extensions.operators import RbfGramOp
from matfree_extensions.util import gp_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VAR_TOL = {torch.float64: 1e-9, torch.float32: 1e-3}  # |var - ref| / s
GRAD_TOL = {torch.float64: 1e-7, torch.float32: 5e-3}  # |g - ref| / max |ref|
SWEEP_TOL = {torch.float64: 1e-12, torch.float32: 1e-5}  # dense sweep against the factored one with L = I


def inv_softplus(v):
    return math.log(math.expm1(v))


def solver(dtype):
    if dtype == torch.float64:
        return cg.cg_adaptive(atol=1e-12, rtol=0.0, maxiter=2000, miniter=1)
    return cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=1000, miniter=1)  # (atol = 0 divides by |x|: entries of x at 0 stop it)


def raw_params(d, ard, dtype=torch.float64):
    ls = [inv_softplus(0.7 + 0.15 * c) for c in range(d)] if ard else inv_softplus(1.1)
    return (torch.tensor(ls, dtype=dtype, device=DEV, requires_grad=True),
            torch.tensor(inv_softplus(0.8), dtype=dtype, device=DEV, requires_grad=True),
            torch.tensor(inv_softplus(0.5), dtype=dtype, device=DEV, requires_grad=True))


def kfun(dist, kind, eps):
    if kind == "rbf":
        return torch.exp(-dist / 2)
    if kind == "matern32":
        r = torch.sqrt(3.0 * dist + eps)
        return (1 + r) * torch.exp(-r)
    return torch.exp(-torch.sqrt(dist + eps))


def kappa0(kind, eps):
    return float(kfun(torch.zeros((), dtype=torch.float64), kind, eps))


def ref_cross(Xa, Xb, ls, s, kind, eps):
    """s K(Xa, Xb) in torch fp64, exactly duplicated pairs at distance 0 (not the expansion's rounding, which Matern-1/2's
    sqrt(dist + eps) would turn into a 1e-8 change of k) and held constant."""
    xa, xb = Xa / ls, Xb / ls
    dist = ((xa * xa).sum(-1)[:, None] + (xb * xb).sum(-1)[None, :] - 2.0 * xa @ xb.T).clamp_min(0.0)
    same = (Xa[:, None, :] == Xb[None, :, :]).all(-1)
    k = kfun(torch.where(same, torch.zeros_like(dist), dist), kind, eps)
    return s * torch.where(same, k.detach(), k)


def ref_var(xs, X, ls, s, nz, kind, eps):
    n = X.shape[0]
    A = ref_cross(X, X, ls, s, kind, eps) + nz * torch.eye(n, dtype=torch.float64, device=DEV)
    Z = torch.linalg.solve_triangular(torch.linalg.cholesky(A), ref_cross(xs, X, ls, s, kind, eps).T, upper=False)
    return s * kappa0(kind, eps) - (Z * Z).sum(0)


def check(got, want, tol, what, floor=0.0):
    """max |got - want| <= tol * max(max |want|, floor): floor = s where a gradient may vanish (a test point on a training point
    far from all others: every term is 0 up to rounding)"""
    err = float((got.double() - want).abs().max()) / max(float(want.abs().max()), floor, 1e-300)
    assert err <= tol, (what, err)


def _problem(d, m, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    X0 = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32).double()  # representable in either dtype
    xs0 = torch.randn(m, d, device=DEV, generator=g, dtype=torch.float32).double()
    xs0[0] = X0[3]  # a test point exactly on a training point
    vbar = torch.randn(m, device=DEV, generator=g, dtype=torch.float32).double()
    return X0, xs0, vbar


# (kernel, ard, dtype, d, m, n): every kernel, both lengthscale forms and dtypes, d in {1, 3, 8, 17, 40} (the register sweeps with
# the shared and the separate lengthscale / input launches and the wide sweep), m in {1, 70, 333} (333 and 70: not a multiple of 64)
CASES = [
    ("rbf", True, torch.float64, 3, 70, 300),
    ("matern32", False, torch.float64, 1, 333, 400),
    ("matern12", True, torch.float64, 8, 1, 300),
    ("rbf", False, torch.float64, 17, 70, 300),
    ("matern32", True, torch.float64, 40, 70, 300),
    ("matern12", False, torch.float64, 40, 333, 200),
    ("rbf", True, torch.float32, 8, 333, 400),
    ("matern32", True, torch.float32, 17, 70, 300),
    ("matern12", False, torch.float32, 3, 70, 300),
    ("rbf", False, torch.float32, 40, 1, 300),
    ("matern32", True, torch.float32, 1, 333, 200),
    ("rbf", True, torch.float64, 11, 70, 300),  # padded d = 12 and 16
    ("matern32", False, torch.float64, 16, 70, 300),
    ("matern32", True, torch.float32, 11, 70, 300),
    ("rbf", False, torch.float32, 16, 70, 300),
]
# (Matern-1/2 at d = 1 is fp64-only: 333 test points among 200 on a line put pairs at distances ~1e-4, where the fp32 expansion's
# rounding of dist (~eps |x|^2) moves the weight exp(-r) / r of the input gradient by tens of percent -- measured 0.23 of the largest
# xs gradient against fp64 -- a property of the distance formula the reference shares, not of the sweep)


@pytest.mark.parametrize("kind,ard,dtype,d,m,n", CASES)
def test_variance_and_gradients_match_fp64_dense(kind, ard, dtype, d, m, n):
    X0, xs0, vbar = _problem(d, m, n, seed=m * 7 + n + d)
    raw = raw_params(d, ard)
    X, xs = X0.clone().requires_grad_(True), xs0.clone().requires_grad_(True)
    var = RbfGramOp(X.to(dtype), kernel=kind).posterior_variance(xs, solver(dtype), *raw)
    assert var.shape == (m,) and var.dtype == dtype
    got = torch.autograd.grad((vbar.to(dtype) * var).sum(), (xs, X, *raw))

    eps = float(torch.finfo(dtype).eps)
    sp = torch.nn.functional.softplus
    Xr, xsr = X0.clone().requires_grad_(True), xs0.clone().requires_grad_(True)
    rr = [r.detach().clone().requires_grad_(True) for r in raw]
    want_var = ref_var(xsr, Xr, sp(rr[0]), sp(rr[1]), sp(rr[2]), kind, eps)
    want = torch.autograd.grad((vbar * want_var).sum(), (xsr, Xr, *rr))
    s = float(sp(raw[1].detach()))
    assert float((var.detach().double() - want_var.detach()).abs().max()) <= VAR_TOL[dtype] * s
    for name, gg, ww in zip(("xs", "X", "raw_l", "raw_s", "raw_noise"), got, want):
        check(gg, ww, GRAD_TOL[dtype], name, floor=s)


def test_matern12_fp32_variance_keeps_kappa0():
    """Far from the data the variance is s kappa(0); for Matern-1/2 in fp32 kappa(0) = exp(-sqrt(eps)) = 1 - 3.5e-4."""
    X0, xs0, _ = _problem(3, 40, 200, seed=5)
    xs0 = xs0 + 8.0
    raw = raw_params(3, True, torch.float32)
    var = RbfGramOp(X0.float(), kernel="matern12").posterior_variance(xs0, solver(torch.float32), *raw)
    sp = torch.nn.functional.softplus
    r64 = [r.detach().double() for r in raw]
    s = float(sp(r64[1]))
    want = ref_var(xs0, X0, sp(r64[0]), sp(r64[1]), sp(r64[2]), "matern12", float(torch.finfo(torch.float32).eps))
    assert float((want - s).abs().min()) > 3e-4 * s  # kappa(0) = 1 would be off by more than the tolerance below
    assert float((var.detach().double() - want).abs().max()) <= 5e-5 * s


def test_gradcheck_fp64():
    g = torch.Generator(device=DEV).manual_seed(3)
    X = torch.randn(30, 2, device=DEV, generator=g, dtype=torch.float64).requires_grad_(True)
    xs = torch.randn(5, 2, device=DEV, generator=g, dtype=torch.float64).requires_grad_(True)
    rl = torch.tensor([0.2, -0.3], dtype=torch.float64, device=DEV, requires_grad=True)
    rs = torch.tensor(0.4, dtype=torch.float64, device=DEV, requires_grad=True)
    rn = torch.tensor(-1.0, dtype=torch.float64, device=DEV, requires_grad=True)
    solve = cg.cg_adaptive(atol=1e-14, rtol=0.0, maxiter=500, miniter=1)

    def f(xs, rl, rs, rn, X):
        return RbfGramOp(X, kernel="matern32").posterior_variance(xs, solve, rl, rs, rn, chunk=2)

    assert torch.autograd.gradcheck(f, (xs, rl, rs, rn, X), eps=1e-6, atol=1e-6, rtol=1e-4)


def _sweep(desc, xs, S, lds, dtype, ls, s, dense=True):
    """(gxs, gls, gs, gX) of one dense sweep, or of the factored mfx_gram_cross_vjp with L = I (m, m), R = S"""
    lib, stream = _lib.get(), _lib.stream_ptr(DEV)
    m = xs.shape[0]
    n, d = desc.n, desc.d
    out = [torch.zeros(m, d, dtype=dtype, device=DEV), torch.zeros_like(ls), torch.zeros_like(s), torch.zeros(n, d, dtype=dtype, device=DEV)]
    st = _lib.OpGrads()
    st.lengthscale, st.outputscale, st.x = out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr()
    if dense:
        ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(C.byref(desc), m)), DEV)
        _lib.check(lib.mfx_gram_cross_vjp_dense(C.byref(desc), _lib.ptr(xs), m, _lib.ptr(S), lds, C.byref(st), _lib.ptr(out[0]),
                                                _lib.ptr(ws), ws.numel(), stream))
    else:
        eye = torch.eye(m, dtype=dtype, device=DEV)
        ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_workspace_bytes(C.byref(desc), m, m)), DEV)
        _lib.check(lib.mfx_gram_cross_vjp(C.byref(desc), _lib.ptr(xs), m, _lib.ptr(eye), m, _lib.ptr(S), lds, m, C.byref(st),
                                          _lib.ptr(out[0]), _lib.ptr(ws), ws.numel(), stream))
    torch.cuda.synchronize()
    return out


# (dtype, kernel, ard, d, m, n, lds): the row form's vector loads (lds % 4 == 0) and scalar loads (odd lds), d <= 16 (one launch),
# padded 32 and wide (separate launches), a small owner set split over many columns
SWEEPS = [
    (torch.float64, "matern32", True, 8, 64, 3000, 3000),
    (torch.float64, "rbf", False, 40, 37, 2049, 2051),
    (torch.float32, "matern12", True, 17, 64, 3000, 3001),
    (torch.float32, "rbf", True, 3, 1024, 700, 704),
    (torch.float32, "matern32", False, 40, 64, 1500, 1500),
]


@pytest.mark.parametrize("dtype,kind,ard,d,m,n,lds", SWEEPS)
def test_dense_sweep_equals_factored_sweep_with_diagonal_L(dtype, kind, ard, d, m, n, lds):
    g = torch.Generator(device=DEV).manual_seed(m + n + d)
    X = torch.randn(n, d, device=DEV, generator=g, dtype=dtype)
    xs = torch.randn(m, d, device=DEV, generator=g, dtype=dtype)
    xs[0] = X[5]
    S = torch.randn(m, lds, device=DEV, generator=g, dtype=dtype)
    raw = raw_params(d, ard, dtype)
    op = RbfGramOp(X, kernel=kind)
    cparams = op.constrain(*(r.detach() for r in raw))
    desc = op.descriptor(cparams, dtype, n)
    dense = _sweep(desc, xs, S, lds, dtype, cparams[0], cparams[1])
    again = _sweep(desc, xs, S, lds, dtype, cparams[0], cparams[1])
    factored = _sweep(desc, xs, S, lds, dtype, cparams[0], cparams[1], dense=False)
    for name, a, b, f in zip(("xs", "lengthscale", "outputscale", "X"), dense, again, factored):
        assert torch.equal(a, b), name  # no atomics: bitwise reproducible
        check(a, f.double(), SWEEP_TOL[dtype], name)


@pytest.mark.parametrize("d", [3, 20, 40])  # one launch (DPAD 4), two launches (DPAD 32), wide with selections
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_dense_sweep_is_bitwise_the_factored_sweep_with_rank_one_weights(dtype, d):
    """batch = 1: the factored sweep forms S_aj = L[a] * R[j], one rounded product; the dense call gets the same products
    materialised by torch in the operator's dtype.  Both entry points are one kernel body with two weight sources, so on equal
    numbers they give equal bits: xs, lengthscale, outputscale and X gradients, torch.equal.  m = 70: a partly dead workgroup with
    dead waves; n = 300: three column splits and a 12-column tail tile; ARD, Matern-3/2, a test point on a training point."""
    m, n = 70, 300
    g = torch.Generator(device=DEV).manual_seed(m + n + d)
    X = torch.randn(n, d, device=DEV, generator=g, dtype=dtype)
    xs = torch.randn(m, d, device=DEV, generator=g, dtype=dtype)
    xs[0] = X[5]
    L = torch.randn(1, m, device=DEV, generator=g, dtype=dtype)
    R = torch.randn(1, n, device=DEV, generator=g, dtype=dtype)
    S = (L.T * R).contiguous()
    op = RbfGramOp(X, kernel="matern32")
    cparams = op.constrain(*(r.detach() for r in raw_params(d, True, dtype)))
    desc = op.descriptor(cparams, dtype, n)
    dense = _sweep(desc, xs, S, n, dtype, cparams[0], cparams[1])
    lib, stream = _lib.get(), _lib.stream_ptr(DEV)
    out = [torch.zeros_like(t) for t in dense]
    st = _lib.OpGrads()
    st.lengthscale, st.outputscale, st.x = out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr()
    ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_workspace_bytes(C.byref(desc), m, 1)), DEV)
    _lib.check(lib.mfx_gram_cross_vjp(C.byref(desc), _lib.ptr(xs), m, _lib.ptr(L), m, _lib.ptr(R), n, 1, C.byref(st), _lib.ptr(out[0]),
                                      _lib.ptr(ws), ws.numel(), stream))
    torch.cuda.synchronize()
    for name, a, f in zip(("xs", "lengthscale", "outputscale", "X"), dense, out):
        assert float(a.abs().max()) > 0, name
        assert torch.equal(a, f), (name, float((a - f).abs().max()))


def test_chunk_size_does_not_change_the_result():
    X0, xs0, vbar = _problem(3, 70, 300, seed=9)
    raw = raw_params(3, True)
    res = []
    for chunk in (1, 7, 64):
        X, xs = X0.clone().requires_grad_(True), xs0.clone().requires_grad_(True)
        var = RbfGramOp(X, kernel="rbf").posterior_variance(xs, solver(torch.float64), *raw, chunk=chunk)
        res.append((var.detach(), *torch.autograd.grad((vbar * var).sum(), (xs, X, *raw))))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.allclose(a, b, rtol=0, atol=1e-10 * float(a.abs().max())), float((a - b).abs().max())


def test_gradients_are_bitwise_reproducible():
    X0, xs0, vbar = _problem(17, 70, 300, seed=13)
    raw = raw_params(17, True, torch.float32)

    def run():
        X, xs = X0.float().requires_grad_(True), xs0.float().requires_grad_(True)
        var = RbfGramOp(X, kernel="matern32").posterior_variance(xs, solver(torch.float32), *raw)
        return torch.autograd.grad((vbar.float() * var).sum(), (xs, X, *raw))

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def _posterior(precond, observation_noise, with_var=True):
    n, m, d = 160, 23, 3
    g = torch.Generator(device=DEV).manual_seed(17)
    X = (torch.rand(n, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2).requires_grad_(True)
    xs = (torch.rand(m, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2)
    xs[2] = X.detach()[7]
    xs.requires_grad_(True)
    y = torch.sin(X.detach().sum(-1))
    c = torch.tensor(0.3, dtype=torch.float64, device=DEV, requires_grad=True)
    rl = torch.tensor([0.1, 0.3, -0.2], dtype=torch.float64, device=DEV, requires_grad=True)
    rs = torch.tensor(0.3, dtype=torch.float64, device=DEV, requires_grad=True)
    rn = torch.tensor(-1.0, dtype=torch.float64, device=DEV, requires_grad=True)
    k_fun, _ = gp_util.kernel_scaled_matern_32(shape_in=(d,), shape_out=())
    m_fun, _ = gp_util.mean_constant(shape_out=())
    constrain = gp_util.constraint_greater_than(1e-2)
    kw = dict(constrain=constrain)
    if with_var:
        kw.update(observation_noise=observation_noise, chunk=8)
    if precond:
        make = gp_util.likelihood_condition_var_p if with_var else gp_util.likelihood_condition_p
        lik, _ = make(gp_util.gram_matvec(), cg.pcg_adaptive(atol=1e-12, rtol=0.0, maxiter=1000, miniter=1),
                      precondition=low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20)), **kw)
    else:
        make = gp_util.likelihood_condition_var if with_var else gp_util.likelihood_condition
        lik, _ = make(gp_util.gram_matvec(), cg.cg_adaptive(atol=1e-12, rtol=0.0, maxiter=1000, miniter=1), **kw)
    post, _ = gp_util.target_posterior(gp_util.model_gp(m_fun, k_fun), lik)(
        X, y, params_mean={"constant_value": c}, params_kernel={"raw_lengthscale": rl, "raw_outputscale": rs},
        params_likelihood={"raw_noise": rn})
    out, info = post(xs)
    return (X, xs, c, rl, rs, rn), y, out, info


@pytest.mark.parametrize("precond,observation_noise", [(True, True), (True, False), (False, True)])
def test_likelihood_condition_var_matches_dense_cholesky(precond, observation_noise):
    inputs, y, (mu, var), info = _posterior(precond, observation_noise)
    X, xs, c, rl, rs, rn = inputs
    _, _, mu_plain, _ = _posterior(precond, observation_noise, with_var=False)
    assert torch.equal(mu.detach(), mu_plain.detach())  # the mean is likelihood_condition[_p]'s, bitwise
    assert int(info["num_clamped"]) == 0
    assert info["variance_solve"]["residual_abs"].shape == (xs.shape[0], X.shape[0])  # one residual per test point
    assert info["variance_solve"]["num_steps"].shape == (xs.shape[0],)
    assert int(info["variance_solve"]["num_steps"].max()) < 1000

    sp = torch.nn.functional.softplus
    eps = float(torch.finfo(torch.float64).eps)
    ls, s, nz = sp(rl), sp(rs), 1e-2 + sp(rn)
    var_ref = ref_var(xs, X, ls, s, nz, "matern32", eps)
    if observation_noise:
        var_ref = var_ref + nz
    assert float((var - var_ref).abs().max()) <= 1e-9 * float(s)
    wts = torch.linspace(0.5, 2.0, xs.shape[0], dtype=torch.float64, device=DEV)
    names = ("X", "xs", "raw_l", "raw_s", "raw_noise")
    got = torch.autograd.grad((wts * var).sum(), (X, xs, rl, rs, rn), retain_graph=True)
    want = torch.autograd.grad((wts * var_ref).sum(), (X, xs, rl, rs, rn), retain_graph=True)
    for name, gg, ww in zip(names, got, want):
        check(gg, ww, GRAD_TOL[torch.float64], name)
    # a loss of both outputs: the mean's gradient still flows next to the variance's
    K = ref_cross(X, X, ls, s, "matern32", eps) + nz * torch.eye(X.shape[0], dtype=torch.float64, device=DEV)
    mu_ref = c + ref_cross(xs, X, ls, s, "matern32", eps) @ torch.cholesky_solve((y - c)[:, None], torch.linalg.cholesky(K))[:, 0]
    got = torch.autograd.grad((mu + wts * var).sum(), (X, xs, c, rl, rs, rn))
    want = torch.autograd.grad((mu_ref + wts * var_ref).sum(), (X, xs, c, rl, rs, rn))
    for name, gg, ww in zip(("X", "xs", "c", "raw_l", "raw_s", "raw_noise"), got, want):
        check(gg, ww, 1e-6, name)
