"""Matern-5/2 (MFX_KERNEL_MATERN52, RbfGramOp(kernel="matern52")) through every Gram path on the GPU.

The oracle under oracle/ does not know this family, so the reference is a dense torch-fp64 kernel matrix written here from

    s = |x/l - y/l|^2 (the |x|^2 + |y|^2 - 2 x.y expansion, clamped at 0),  r = sqrt(5 s + eps),  k = sigma (1 + r + r^2/3) exp(-r)

with exactly duplicated pairs at distance 0 and held constant, and the eps of the dtype UNDER TEST passed in (the style of ref_cross
in tests/test_gpu_posterior_grad.py); its gradients come from torch autograd.  Every tolerance is the one the Matern-3/2 case of the
same kind uses, cited next to it."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, cg, hutchinson, lanczos, low_rank
    from matfree_extensions.operators import RbfGramOp
    from matfree_extensions.util import gp_util

DEV = torch.device("cuda:0")
KIND = "matern52"
MINVAL = 1e-4
sp = torch.nn.functional.softplus


def k52(dist, eps):
    r = torch.sqrt(5.0 * dist + eps)
    return (1 + r + r * r / 3) * torch.exp(-r)


def ref_cross(Xa, Xb, ls, s, eps):
    """s K(Xa, Xb) in torch fp64: distance expansion, clamp at 0, exactly duplicated pairs at distance 0 and held constant."""
    xa, xb = Xa / ls, Xb / ls
    dist = ((xa * xa).sum(-1)[:, None] + (xb * xb).sum(-1)[None, :] - 2.0 * xa @ xb.T).clamp_min(0.0)
    same = torch.ones(dist.shape, dtype=torch.bool, device=dist.device)
    for c in range(Xa.shape[1]):  # (column by column: no (m, n, d) temporary at n = 36 584)
        same &= Xa.detach()[:, c, None] == Xb.detach()[None, :, c]
    k = k52(torch.where(same, torch.zeros_like(dist), dist), eps)
    return s * torch.where(same, k.detach(), k)


def ref_gram(X, raw, eps, minval=MINVAL):
    n = X.shape[0]
    return ref_cross(X, X, sp(raw[0]), sp(raw[1]), eps) + (minval + sp(raw[2])) * torch.eye(n, dtype=torch.float64, device=X.device)


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def close(a, b, rtol, atol_rel=None):
    """tests/test_gpu_parity.py:36-42 on tensors: |a - b| <= atol_rel max|b| + rtol |b|"""
    a, b = a.detach().double(), b.detach().double()
    atol = (atol_rel if atol_rel is not None else rtol) * max(float(b.abs().max()), 1e-300)
    err = float(((a - b).abs() - rtol * b.abs()).max())
    print(f"    max abs err {float((a - b).abs().max()):.3e}  scale {float(b.abs().max()):.3e}  allowed {atol:.3e}")
    return err <= atol


def problem(n, d, p, ard, dtype, seed, wide=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) * (1.5 / np.sqrt(d) if wide else 1.0)  # tests/test_gpu_parity.py:160: distances O(1) at large d
    raw = (rng.standard_normal(d) * 0.3 + 0.5 if ard else np.array(0.7), np.array(0.4), np.array(-1.0))
    V, Cc = rng.standard_normal((p, n)), rng.standard_normal((p, n))
    # what the operator under test sees: inputs and raw parameters rounded to its dtype
    X = T(X, dtype).double()
    raw = [T(r, dtype).double() for r in raw]
    return X, raw, T(V, dtype).double(), T(Cc, dtype).double()


def check_apply_and_sweep(n, d, p, ard, dtype, precision, tol, seed, wide=False, grads=True):
    """matvec, its transpose through autograd and the three parameter gradients, as tests/test_gpu_parity.py:123-141 checks Matern-3/2"""
    X, raw, V, Cc = problem(n, d, p, ard, dtype, seed, wide)
    eps = float(torch.finfo(dtype).eps)
    op = RbfGramOp(X.to(dtype), noise_minval=MINVAL, precision=precision, kernel=KIND)
    params = [r.to(dtype).requires_grad_(True) for r in raw]
    Vt = V.to(dtype).requires_grad_(True)
    y = op(Vt, *params)
    rr = [r.clone().requires_grad_(True) for r in raw]
    A = ref_gram(X, rr, eps)
    want = V @ A.T
    assert close(y, want, tol), "matvec"  # tests/test_gpu_parity.py:134
    if not grads:
        return
    got = torch.autograd.grad(y, (Vt, *params), Cc.to(dtype))
    assert close(got[0], Cc @ A, tol), "transpose"  # tests/test_gpu_parity.py:136
    ref = torch.autograd.grad((Cc * want).sum(), rr)
    gtol = tol * (50 if dtype == torch.float32 else 10)  # tests/test_gpu_parity.py:138
    for name, g, r in zip(("raw_l", "raw_s", "raw_noise"), got[1:], ref):
        assert close(g.reshape(r.shape), r, gtol, atol_rel=gtol * math.sqrt(n)), name  # tests/test_gpu_parity.py:140


MODES = [(torch.float64, 1e-11, "fp32"), (torch.float32, 5e-5, "fp32"), (torch.float32, 5e-5, "f16x3-matvec"),
         (torch.float32, 5e-5, "f16x3")]  # tests/test_gpu_parity.py:110-111


@pytest.mark.parametrize("dtype,tol,precision", MODES)
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("n,d,p", [(300, 1, 1), (515, 3, 5), (700, 8, 8), (700, 9, 8), (640, 8, 64), (1000, 16, 40), (2100, 3, 40),
                                   (2304, 9, 3), (700, 3, 33), (2050, 16, 33), (2304, 12, 65)])
def test_apply_and_param_sweep_split_tiers(dtype, tol, precision, ard, n, d, p):
    """d <= 16: the split (3 x f16) matvec and gradient GEMM in the f16x3 modes, exact fp32 matrix cores in "fp32", VALU for few
    vectors at small n, fp64 VALU; p <= 32, p > 32 and two probe chunks (p = 65)."""
    check_apply_and_sweep(n, d, p, ard, dtype, precision, tol, seed=2)


@pytest.mark.parametrize("dtype,tol,precision", [MODES[0], MODES[1], MODES[3]])  # tests/test_gpu_parity.py:143
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("n,d,p", [(600, 20, 8), (2304, 32, 3), (900, 20, 40), (777, 17, 33), (300, 33, 3), (520, 40, 8), (1000, 40, 70),
                                   (2100, 64, 5), (515, 90, 8), (2100, 128, 5), (640, 97, 70), (300, 129, 8), (260, 200, 5)])
def test_apply_and_param_sweep_wide_tiers(dtype, tol, precision, ard, n, d, p):
    """16 < d <= 32 (h3 kernel with DPAD = 32, exact-fp32 sweep), d in {40, 90, 97, 128}: exact-fp32 matrix-core matvec, sweep on the
    matrix cores up to padded 64 and VALU beyond; d > 128: VALU."""
    check_apply_and_sweep(n, d, p, ard, dtype, precision, tol, seed=d, wide=True)


@pytest.mark.parametrize("n,d,p,ard,precision", [(4099, 9, 64, True, "f16x3"), (4099, 3, 17, False, "f16x3-matvec"), (4099, 20, 8, True, "fp32"),
                                                 (4099, 40, 8, False, "f16x3")])
def test_ragged_n_with_gradients(n, d, p, ard, precision):
    check_apply_and_sweep(n, d, p, ard, torch.float32, precision, 5e-5, seed=5, wide=d > 16)  # tests/test_gpu_parity.py:110


@pytest.mark.parametrize("p", [64, 5])
def test_matvec_at_the_small_benchmark_size(p):
    """n = 36 584, d = 9 (tools/bench_matvec_small.py): pre-packed tiles with 64 vectors, in-kernel split with 5"""
    check_apply_and_sweep(36584, 9, p, False, torch.float32, "f16x3", 5e-5, seed=9, grads=False)  # tests/test_gpu_parity.py:110


def _apply_block(op, cparams, V, row0, nrows, kernel_fn=None, y=None):
    p, n = V.shape
    desc = op.descriptor(cparams, V.dtype, n)
    desc.row0, desc.nrows = row0, nrows
    if kernel_fn is not None:
        desc.kernel_fn = kernel_fn
    ws = _lib.workspace(desc, n, 1, p, V.device)
    y = torch.empty((p, nrows or n), dtype=V.dtype, device=V.device) if y is None else y
    rc = _lib.get().mfx_op_apply(C.byref(desc), _lib.ptr(V), n, _lib.ptr(y), nrows or n, p, 0, _lib.ptr(ws), ws.numel(),
                                 _lib.stream_ptr(V.device))
    return rc, y


@pytest.mark.parametrize("dtype,tol,precision,d,p", [(torch.float32, 5e-5, "f16x3", 8, 40), (torch.float32, 5e-5, "fp32", 40, 8),
                                                     (torch.float64, 1e-11, "fp32", 3, 5)])
def test_row_block(dtype, tol, precision, d, p):
    n, row0, nrows = 2500, 640, 1001
    X, raw, V, _ = problem(n, d, p, True, dtype, seed=3, wide=d > 16)
    op = RbfGramOp(X.to(dtype), noise_minval=MINVAL, precision=precision, kernel=KIND)
    rc, y = _apply_block(op, op.constrain(*[r.to(dtype) for r in raw]), V.to(dtype), row0, nrows)
    assert rc == 0
    want = V @ ref_gram(X, raw, float(torch.finfo(dtype).eps)).T
    assert close(y, want[:, row0:row0 + nrows], tol)  # tests/test_gpu_sharded.py:71 (row blocks equal the rows of the whole operator)


@pytest.mark.parametrize("bad", [4, -1, 1 << 20])
@pytest.mark.parametrize("dtype,p", [(torch.float32, 40), (torch.float32, 1), (torch.float64, 3)])
def test_unknown_kernel_fn_is_refused_before_any_launch(bad, dtype, p):
    n, d = 700, 3
    X, raw, V, _ = problem(n, d, p, False, dtype, seed=4)
    op = RbfGramOp(X.to(dtype), noise_minval=MINVAL, kernel=KIND)
    y = torch.full((p, n), 123.0, dtype=dtype, device=DEV)
    rc, y = _apply_block(op, op.constrain(*[r.to(dtype) for r in raw]), V.to(dtype), 0, 0, kernel_fn=bad, y=y)
    torch.cuda.synchronize()
    assert rc == -1  # MFX_ERR_INVALID
    assert b"kernel_fn" in _lib.get().mfx_last_error()
    assert bool((y == 123.0).all())  # nothing was written
    rc, _ = _apply_block(op, op.constrain(*[r.to(dtype) for r in raw]), V.to(dtype), 0, 0, kernel_fn=3, y=y)
    assert rc == 0


def lanczos_quadform_dense(A, v, k):
    """v^T log(A) v by k steps of Lanczos with full reorthogonalisation on the dense matrix, differentiable by autograd"""
    nv = torch.linalg.vector_norm(v)
    Q = [v / nv]
    al, be = [], []
    for j in range(k):
        w = A @ Q[j]
        al.append(w @ Q[j])
        Qm = torch.stack(Q)
        w = w - Qm.T @ (Qm @ w)
        w = w - Qm.T @ (Qm @ w)
        if j + 1 < k:
            be.append(torch.linalg.vector_norm(w))
            Q.append(w / be[-1])
    Tm = torch.diag(torch.stack(al)) + torch.diag(torch.stack(be), 1) + torch.diag(torch.stack(be), -1)
    lam, U = torch.linalg.eigh(Tm)
    return nv * nv * (U[0] ** 2 * torch.log(lam)).sum()


@pytest.mark.parametrize("dtype,precision,vtol,gtol", [(torch.float64, "fp32", 1e-9, 1e-7), (torch.float32, "f16x3", 1e-4, 2e-3),
                                                       (torch.float32, "fp32", 1e-4, 2e-3)])  # tests/test_gpu_parity.py:2-4
@pytest.mark.parametrize("n,d,p,ard", [(600, 8, 32, False), (600, 8, 32, True), (2100, 3, 4, True), (640, 20, 16, True), (520, 40, 16, False),
                                       (520, 50, 16, True), (515, 90, 16, True), (300, 200, 4, False)])
def test_slq_value_and_parameter_gradients(dtype, precision, vtol, gtol, n, d, p, ard):
    """lanczos.integrand_spd(log) on a batch of probes against Lanczos on the dense fp64 matrix, value and all three gradients"""
    k = 10
    X, raw, V, _ = problem(n, d, p, ard, dtype, seed=n + d, wide=d > 16)
    V = torch.sign(V)
    op = RbfGramOp(X.to(dtype), noise_minval=MINVAL, precision=precision, kernel=KIND)
    params = [r.to(dtype).requires_grad_(True) for r in raw]
    value = lanczos.integrand_spd(torch.log, k, op)(V.to(dtype), *params).sum()
    got = torch.autograd.grad(value, params)
    rr = [r.clone().requires_grad_(True) for r in raw]
    A = ref_gram(X, rr, float(torch.finfo(dtype).eps))
    want = sum(lanczos_quadform_dense(A, v, k) for v in V)
    ref = torch.autograd.grad(want, rr)
    print(f"    value {float(value):.8e} want {float(want):.8e}")
    assert abs(float(value) - float(want)) <= vtol * abs(float(want))
    for name, g, r in zip(("raw_l", "raw_s", "raw_noise"), got, ref):
        assert close(g.reshape(r.shape), r, gtol), name


# ---- inputs X: tests/test_gpu_input_grad.py:23 (TOL per dtype, error against the absolute term sums of each element)
XTOL = {torch.float64: 1e-9, torch.float32: 1e-3}


@pytest.mark.parametrize("dtype,precision,d,n,batch,ard,dups", [(torch.float64, "f16x3", 8, 300, 3, True, True), (torch.float32, "f16x3", 8, 2100, 3, True, False),
                                                                (torch.float32, "f16x3", 16, 4099, 16, False, False), (torch.float32, "f16x3", 40, 300, 16, True, True),
                                                                (torch.float64, "f16x3", 40, 127, 16, False, False), (torch.float32, "fp32", 1, 700, 1, False, False)])
def test_matvec_vjp_wrt_inputs(dtype, precision, d, n, batch, ard, dups):
    g = torch.Generator(device=DEV).manual_seed(n * 31 + d)
    X0 = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32).double()
    if dups:
        X0[1] = X0[0]
        X0[n // 2] = X0[n - 1]
    U = torch.randn(batch, n, device=DEV, generator=g, dtype=torch.float32).to(dtype)
    V = torch.randn(batch, n, device=DEV, generator=g, dtype=torch.float32).to(dtype)
    ls = T([0.7 + 0.15 * c for c in range(d)] if ard else 1.1)
    raw = [torch.log(torch.expm1(ls)), T(math.log(math.expm1(0.8))), T(math.log(math.expm1(0.3)))]
    X = X0.clone().requires_grad_(True)
    op = RbfGramOp(X.to(dtype), precision=precision, kernel=KIND)
    (gx,) = torch.autograd.grad((U * op(V, *raw)).sum(), X)
    eps = float(torch.finfo(dtype).eps)
    lsd, s = sp(raw[0]).to(dtype).double().reshape(-1), sp(raw[1]).to(dtype).double()
    Xr = X0.clone().requires_grad_(True)
    S = U.double().T @ V.double()
    (gref,) = torch.autograd.grad((S * ref_cross(Xr, Xr, lsd, s, eps)).sum(), Xr)
    with torch.no_grad():  # absolute term sums: sum_j |S_ij + S_ji| s w_ij (|xs_ic| + |xs_jc|) / l_c   (tests/test_gpu_input_grad.py:57-74)
        xs = X0 / lsd
        dist = (xs[:, None, :] - xs[None, :, :]).pow(2).sum(-1)
        r = torch.sqrt(5 * dist + eps)
        W = (S.abs() + S.abs().T) * (5.0 / 3.0) * (1 + r) * torch.exp(-r)
        scale = ((W[:, :, None] * (xs.abs()[:, None, :] + xs.abs()[None, :, :])).sum(1) * s / lsd.expand(d))
    err = (gx - gref).abs() / (scale + 1e-300)
    print(f"    max err / term sum {float(err.max()):.3e}")
    assert float(err.max()) <= XTOL[dtype]


# ---- cross-covariance matvec and the predictive variance
CTOL = {torch.float64: 1e-9, torch.float32: 1e-3}  # tests/test_gpu_posterior_grad.py:23
VAR_TOL = {torch.float64: 1e-9, torch.float32: 1e-3}  # tests/test_gpu_posterior_var.py:22
GRAD_TOL = {torch.float64: 1e-7, torch.float32: 5e-3}  # tests/test_gpu_posterior_var.py:23


def _cross_problem(d, m, n, p, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    X0 = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32).double()
    Xn0 = torch.randn(m, d, device=DEV, generator=g, dtype=torch.float32).double()
    Xn0[0] = X0[3]  # a test point exactly on a training point
    V = torch.randn(p, n, device=DEV, generator=g, dtype=torch.float32).double()
    Ybar = torch.randn(p, m, device=DEV, generator=g, dtype=torch.float32).double()
    return X0, Xn0, V, Ybar


def _raw(d, ard, noise=0.3):
    inv = lambda v: math.log(math.expm1(v))  # noqa: E731
    ls = [inv(0.7 + 0.15 * c) for c in range(d)] if ard else inv(1.1)
    return [T(ls, grad=True), T(inv(0.8), grad=True), T(inv(noise), grad=True)]


@pytest.mark.parametrize("ard,dtype,d,m,n,p", [(False, torch.float64, 1, 333, 2049, 1), (True, torch.float64, 17, 333, 700, 9), (True, torch.float64, 40, 70, 700, 3),
                                               (True, torch.float32, 17, 1, 2049, 1), (True, torch.float32, 8, 333, 2049, 9), (False, torch.float32, 40, 70, 700, 9)])
def test_cross_apply_forward_transpose_and_five_gradients(ard, dtype, d, m, n, p):
    X0, Xn0, V0, Ybar = _cross_problem(d, m, n, p, dtype, seed=m * 7 + n + d)
    raw = _raw(d, ard)
    X, Xn = X0.clone().requires_grad_(True), Xn0.clone().requires_grad_(True)
    V = V0.to(dtype).requires_grad_(True)
    y = RbfGramOp(X.to(dtype), kernel=KIND).cross_apply(Xn, V, *raw)
    assert y.shape == (p, m) and y.dtype == dtype
    got = torch.autograd.grad((Ybar.to(dtype) * y).sum(), (V, Xn, X, raw[0], raw[1]))

    eps = float(torch.finfo(dtype).eps)
    ls = sp(raw[0]).detach().to(dtype).double().reshape(-1).requires_grad_(True)
    s = sp(raw[1]).detach().to(dtype).double().requires_grad_(True)
    Xr, Xnr, Vr = X0.clone().requires_grad_(True), Xn0.clone().requires_grad_(True), V0.clone().requires_grad_(True)
    Kx = ref_cross(Xnr, Xr, ls, s, eps)
    want_y = Vr @ Kx.T
    want = torch.autograd.grad((Ybar * want_y).sum(), (Vr, Xnr, Xr, ls, s))
    with torch.no_grad():  # absolute term sums of every element (tests/test_gpu_posterior_grad.py:54-77)
        k_abs = Kx.abs()
        assert float(((y.double() - want_y).abs() / (V0.abs() @ k_abs.T + 1e-300)).max()) <= CTOL[dtype]  # forward
        S = Ybar.T @ V0
        xa, xb = Xn0 / ls, X0 / ls
        diff = xa[:, None, :] - xb[None, :, :]
        r = torch.sqrt(5 * (diff * diff).sum(-1) + eps)
        W = S.abs() * (5.0 / 3.0) * (1 + r) * torch.exp(-r)
        mag = xa.abs()[:, None, :] + xb.abs()[None, :, :]
        lsv = ls.expand(d)
        scales = (Ybar.abs() @ k_abs,  # transpose: K(X, X_new) ybar
                  (W[:, :, None] * mag).sum(1) * s / lsv, (W[:, :, None] * mag).sum(0) * s / lsv,
                  (W[:, :, None] * diff * diff).sum((0, 1)) * s / lsv, (S.abs() * k_abs / s).sum())
    dls = torch.sigmoid(raw[0].detach()).reshape(-1)  # raw -> constrained
    dsc = torch.sigmoid(raw[1].detach())
    got = list(got)
    got[3] = got[3].reshape(-1).double() / dls if ard else got[3].double() / dls
    want = list(want)
    if not ard:
        want[3], scales = want[3].sum(), (*scales[:3], scales[3].sum(), scales[4])
    got[4] = got[4].double() / dsc
    for name, g, w, sc in zip(("v", "xnew", "X", "lengthscale", "outputscale"), got, want, scales):
        err = float(((g.double().reshape(w.shape) - w).abs() / (sc + 1e-300)).max())
        print(f"    {name}: {err:.3e}")
        assert err <= CTOL[dtype], name


def _solver(dtype):  # tests/test_gpu_posterior_var.py:31-34
    if dtype == torch.float64:
        return cg.cg_adaptive(atol=1e-12, rtol=0.0, maxiter=2000, miniter=1)
    return cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=1000, miniter=1)


def ref_var(xs, X, ls, s, nz, eps):
    A = ref_cross(X, X, ls, s, eps) + nz * torch.eye(X.shape[0], dtype=torch.float64, device=DEV)
    Z = torch.linalg.solve_triangular(torch.linalg.cholesky(A), ref_cross(xs, X, ls, s, eps).T, upper=False)
    kappa0 = float(k52(torch.zeros((), dtype=torch.float64), eps))
    return s * kappa0 - (Z * Z).sum(0)


@pytest.mark.parametrize("ard,dtype,d,m,n", [(False, torch.float64, 1, 333, 400), (True, torch.float64, 40, 70, 300), (True, torch.float32, 17, 70, 300),
                                             (True, torch.float32, 3, 70, 300), (False, torch.float32, 40, 70, 200)])
def test_posterior_variance_and_gradients(ard, dtype, d, m, n):
    X0, xs0, _, _ = _cross_problem(d, m, n, 1, dtype, seed=m * 7 + n + d)
    if m > 2:
        xs0[1] = 50.0  # far from the data: the variance is s kappa(0)
    vbar = torch.linspace(0.5, 2.0, m, dtype=torch.float64, device=DEV)
    raw = _raw(d, ard, noise=0.5)
    X, xs = X0.clone().requires_grad_(True), xs0.clone().requires_grad_(True)
    var = RbfGramOp(X.to(dtype), kernel=KIND).posterior_variance(xs, _solver(dtype), *raw)
    assert var.shape == (m,) and var.dtype == dtype
    got = torch.autograd.grad((vbar.to(dtype) * var).sum(), (xs, X, *raw))
    eps = float(torch.finfo(dtype).eps)
    Xr, xsr = X0.clone().requires_grad_(True), xs0.clone().requires_grad_(True)
    rr = [r.detach().clone().requires_grad_(True) for r in raw]
    want_var = ref_var(xsr, Xr, sp(rr[0]), sp(rr[1]), sp(rr[2]), eps)
    want = torch.autograd.grad((vbar * want_var).sum(), (xsr, Xr, *rr))
    s = float(sp(raw[1].detach()))
    r0 = math.sqrt(eps)
    if m > 2:
        assert abs(float(var[1]) - s * (1 + r0 + r0 * r0 / 3) * math.exp(-r0)) <= VAR_TOL[dtype] * s
    assert float((var.detach().double() - want_var.detach()).abs().max()) <= VAR_TOL[dtype] * s  # tests/test_gpu_posterior_var.py:124
    for name, gg, ww in zip(("xs", "X", "raw_l", "raw_s", "raw_noise"), got, want):
        err = float((gg.double().reshape(ww.shape) - ww).abs().max()) / max(float(ww.abs().max()), s)
        print(f"    {name}: {err:.3e}")
        assert err <= GRAD_TOL[dtype], name  # tests/test_gpu_posterior_var.py:83-87, 126


def test_partial_cholesky_preconditioner_and_pcg_against_a_dense_solve():
    n, d, rank = 500, 3, 24
    rng = np.random.default_rng(2)
    X = T(rng.uniform(-1, 1, (n, d)))
    raw = [T(0.2), T(0.4), T(-3.0)]
    eps = float(torch.finfo(torch.float64).eps)
    A = ref_gram(X, raw, eps)
    bound = RbfGramOp(X, noise_minval=MINVAL, kernel=KIND).bind(*raw)
    L, info = low_rank.cholesky_partial_pivot(rank=rank)(low_rank.without_noise(bound), n)
    # against the greedy (largest remaining diagonal) pivoted Cholesky of the dense fp64 matrix, written out here
    K = A - (MINVAL + sp(raw[2])) * torch.eye(n, dtype=torch.float64, device=DEV)
    diag, Lref, piv_ref = torch.diagonal(K).clone(), torch.zeros(rank, n, dtype=torch.float64, device=DEV), []
    for i in range(rank):
        j = int(diag.argmax())
        piv_ref.append(j)
        Lref[i] = (K[j] - Lref[:i].T @ Lref[:i, j]) / torch.sqrt(diag[j])
        diag = diag - Lref[i] ** 2
    Lm = L if L.shape[0] == n else L.T
    assert [int(q) for q in info["pivots"]] == piv_ref
    assert close(Lm @ Lm.T, Lref.T @ Lref, 1e-8, atol_rel=1e-9)  # tests/test_gpu_next_tier.py:268-269 (rtol 1e-8, atol 1e-9)
    pre, pinfo = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank))(low_rank.without_noise(bound), n)
    assert bool(pinfo["success"])
    b = T(rng.standard_normal(n))
    want = torch.linalg.solve(A, b)
    kw = dict(atol=1e-10, rtol=0.0, maxiter=400, miniter=3)
    noise = MINVAL + sp(raw[2])
    x, xinfo = cg.pcg_adaptive(**kw)(bound, b, pre.bind(noise))
    x0, info0 = cg.cg_adaptive(**kw)(bound, b)
    assert close(x, want, 1e-5)  # tests/test_gpu_next_tier.py:300
    assert int(xinfo["num_steps"]) < int(info0["num_steps"])  # the preconditioner earns its keep


@pytest.mark.parametrize("dtype,vtol,gtol", [(torch.float64, 1e-6, 2e-5), (torch.float32, 1e-4, 5e-3)])  # tests/test_gpu_next_tier.py:340
def test_target_logml_krylov_p_against_dense_cholesky(dtype, vtol, gtol):
    """SLQ + preconditioned CG behind target_logml against logpdf_cholesky ON THE SAME OPERATOR family at small n: with the Krylov depth
    at n the quadrature is exact up to the probes, so the probes are what remains -- compare instead with the dense fp64 formulas for the
    solve and with Lanczos on the dense matrix for the log-determinant."""
    rng = np.random.default_rng(4)
    n, d, k, nprobes, rank, steps = 384, 3, 12, 8, 16, 60
    X = rng.uniform(-1, 1, (n, d))
    y = np.sin(X.sum(-1)) + 0.1 * rng.standard_normal(n)
    minval, cval, seed = 1e-3, 0.25, 11
    k_fun, _ = gp_util.kernel_scaled_matern_52(shape_in=(d,), shape_out=())
    m_fun, _ = gp_util.mean_constant(shape_out=())
    sample = hutchinson.sampler_rademacher(torch.empty(n, dtype=dtype, device=DEV), num=nprobes)
    logdet = gp_util.krylov_logdet_slq(k, sample=sample, num_batches=1)
    logpdf_p = gp_util.logpdf_krylov_p(solve_p=cg.pcg_fixed_step(steps), logdet=logdet)
    precondition = low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=rank))
    constrain = gp_util.constraint_greater_than(minval)
    lik, _ = gp_util.likelihood_pdf_p(gp_util.gram_matvec(precision="f16x3-matvec"), logpdf_p, precondition, constrain=constrain)
    loss = gp_util.target_logml(gp_util.model_gp(m_fun, k_fun), lik)
    tl, ts, tn, tc = T(0.1, dtype, True), T(0.3, dtype, True), T(-2.0, dtype, True), T(cval, dtype, True)
    kw = dict(params_mean={"constant_value": tc}, params_kernel={"raw_lengthscale": tl, "raw_outputscale": ts},
              params_likelihood={"raw_noise": tn})
    value, info = loss(T(X, dtype), T(y, dtype), seed, **kw)
    got = torch.autograd.grad(value, (tl, ts, tn, tc))
    assert bool(info["precondition"]["success"])

    # dense fp64: -1/2 (b^T A^-1 b + logdet_slq + n log 2 pi) with the same probes
    rr = [T(0.1, grad=True), T(0.3, grad=True), T(-2.0, grad=True)]
    rc = T(cval, grad=True)
    A = ref_gram(T(X, dtype).double(), rr, float(torch.finfo(dtype).eps), minval=minval)
    b = T(y, dtype).double() - rc
    probes = sample(seed).double()
    ld = sum(lanczos_quadform_dense(A, v, k) for v in probes) / nprobes
    want = -0.5 * (b @ torch.linalg.solve(A, b) + ld + n * math.log(2 * math.pi))
    ref = torch.autograd.grad(want, (*rr, rc))
    print(f"    value {float(value):.8e} want {float(want):.8e}")
    assert abs(float(value) - float(want)) <= vtol * abs(float(want))
    for name, g, w in zip(("raw_l", "raw_s", "raw_noise", "c"), got, ref):
        print(f"    {name}: {float(g):.6e} want {float(w):.6e}")
        assert abs(float(g) - float(w)) <= gtol * max(abs(float(w)), 1.0), name  # tests/test_gpu_next_tier.py:391

    # and the dense Cholesky likelihood of the library on the same operator: the exact value next to the fp64 formulas
    lik_c, _ = gp_util.likelihood_pdf(gp_util.gram_matvec(), gp_util.logpdf_cholesky(), constrain=constrain)
    kw64 = dict(params_mean={"constant_value": T(cval)}, params_kernel={"raw_lengthscale": T(0.1), "raw_outputscale": T(0.3)},
                params_likelihood={"raw_noise": T(-2.0)})
    vchol, _ = gp_util.target_logml(gp_util.model_gp(m_fun, k_fun), lik_c)(T(X), T(y), **kw64)
    A64 = ref_gram(T(X), [T(0.1), T(0.3), T(-2.0)], float(torch.finfo(torch.float64).eps), minval=minval)
    b64 = T(y) - cval
    exact = -0.5 * (b64 @ torch.linalg.solve(A64, b64) + torch.logdet(A64) + n * math.log(2 * math.pi))
    assert abs(float(vchol) - float(exact)) <= 1e-9 * abs(float(exact))


def test_likelihood_condition_var_p_mean_and_variance():
    """tests/test_gpu_posterior_var.py:236-296 with the new kernel: mean and variance against the dense formulas"""
    n, m, d = 300, 40, 3
    g = torch.Generator(device=DEV).manual_seed(3)
    X = (torch.rand(n, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2).requires_grad_(True)
    xs = torch.rand(m, d, device=DEV, generator=g, dtype=torch.float64) * 4 - 2
    xs[2] = X.detach()[7]
    xs.requires_grad_(True)
    y = torch.sin(X.detach().sum(-1))
    c, rl = T(0.3, grad=True), T([0.1, 0.3, -0.2], grad=True)
    rs, rn = T(0.3, grad=True), T(-1.0, grad=True)
    k_fun, _ = gp_util.kernel_scaled_matern_52(shape_in=(d,), shape_out=())
    m_fun, _ = gp_util.mean_constant(shape_out=())
    lik, _ = gp_util.likelihood_condition_var_p(gp_util.gram_matvec(), cg.pcg_adaptive(atol=1e-12, rtol=0.0, maxiter=1000, miniter=1),
                                                precondition=low_rank.preconditioner(low_rank.cholesky_partial_pivot(rank=20)),
                                                constrain=gp_util.constraint_greater_than(1e-2), observation_noise=True, chunk=8)
    post, _ = gp_util.target_posterior(gp_util.model_gp(m_fun, k_fun), lik)(
        X, y, params_mean={"constant_value": c}, params_kernel={"raw_lengthscale": rl, "raw_outputscale": rs},
        params_likelihood={"raw_noise": rn})
    (mu, var), info = post(xs)
    eps = float(torch.finfo(torch.float64).eps)
    ls, s, nz = sp(rl), sp(rs), 1e-2 + sp(rn)
    var_ref = ref_var(xs, X, ls, s, nz, eps) + nz
    K = ref_cross(X, X, ls, s, eps) + nz * torch.eye(n, dtype=torch.float64, device=DEV)
    mu_ref = c + ref_cross(xs, X, ls, s, eps) @ torch.cholesky_solve((y - c)[:, None], torch.linalg.cholesky(K))[:, 0]
    assert float((var - var_ref).abs().max()) <= 1e-9 * float(s)  # tests/test_gpu_posterior_var.py:284
    assert float((mu - mu_ref).abs().max()) <= 1e-9 * float(mu_ref.abs().max())
    wts = torch.linspace(0.5, 2.0, m, dtype=torch.float64, device=DEV)
    got = torch.autograd.grad((mu + wts * var).sum(), (X, xs, c, rl, rs, rn))
    want = torch.autograd.grad((mu_ref + wts * var_ref).sum(), (X, xs, c, rl, rs, rn))
    for name, gg, ww in zip(("X", "xs", "c", "raw_l", "raw_s", "raw_noise"), got, want):
        err = float((gg - ww).abs().max()) / float(ww.abs().max())
        print(f"    {name}: {err:.3e}")
        assert err <= 1e-6, name  # tests/test_gpu_posterior_var.py:299


def test_hipgraph_replay_of_a_launch_bound_shape_gives_the_eager_result():
    """a launch-bound shape (small n, few probes) called again and again, as tests/test_gpu_graphs.py:84-108 does for the dense
    operator: forward and adjoint are captured and replayed, every call gives the first call's bits, and those match the reference"""
    n, d, k, p = 256, 3, 8, 2
    X, raw, V, _ = problem(n, d, p, True, torch.float64, seed=8)
    V = torch.sign(V)
    integrand = lanczos.integrand_spd(torch.log, k, RbfGramOp(X, noise_minval=MINVAL, kernel=KIND))
    bufs = [r.clone().requires_grad_(True) for r in raw]
    first = None
    cap0, rep0 = _lib.graph_stats()
    for it in range(5):
        value = integrand(V, *bufs).sum()
        grads = torch.autograd.grad(value, bufs)
        got = [t.detach().clone() for t in (value, *grads)]
        if first is None:
            first = got
        else:
            for a, b in zip(got, first):
                assert torch.equal(a, b)
        del value, grads, got  # outputs go back to the allocator: the next call gets the same addresses
    cap1, rep1 = _lib.graph_stats()
    assert cap1 - cap0 >= 1 and rep1 - rep0 >= 2  # tests/test_gpu_graphs.py:108
    rr = [b.detach().clone().requires_grad_(True) for b in bufs]
    A = ref_gram(X, rr, float(torch.finfo(torch.float64).eps))
    want = sum(lanczos_quadform_dense(A, v, k) for v in V)
    ref = torch.autograd.grad(want, rr)
    assert abs(float(first[0]) - float(want)) <= 1e-9 * abs(float(want))  # tests/test_gpu_parity.py:2 (fp64: 1e-9 / 1e-7)
    for g, r in zip(first[1:], ref):
        assert close(g.reshape(r.shape), r, 1e-7)


def _sharded_worker(rank, world, port, out):
    import datetime
    import os

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from matfree_extensions.distributed import slq_value_and_grad

    op, params = _sharded_problem()
    mean, std, grads = slq_value_and_grad(op, torch.log, 10, params, n=858, seed=3, num_probes=8, row_group_size=world,
                                          dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    if rank == world - 1:
        torch.save({"mean": mean.cpu(), "grads": [g.cpu() for g in grads]}, out)
    dist.barrier()
    dist.destroy_process_group()


def _sharded_problem():
    g = torch.Generator().manual_seed(0)
    X = torch.randn((858, 8), generator=g, dtype=torch.float64).float().to(DEV)
    params = [torch.full((8,), 0.9, device=DEV), torch.tensor(0.3, device=DEV), torch.tensor(-1.0, device=DEV)]
    return gp_util.gram_operator(X, noise_minval=MINVAL, precision="f16x3", kernel=KIND), [q.requires_grad_(True) for q in params]


def test_two_row_shards_reproduce_the_single_process_estimate(tmp_path):
    """tests/test_gpu_sharded.py:169-190 with the new kernel: two processes, one row shard each (the second ragged)"""
    import socket

    import torch.multiprocessing as mp

    from matfree_extensions.distributed import slq_value_and_grad

    op, params = _sharded_problem()
    mean, _, grads = slq_value_and_grad(op, torch.log, 10, params, n=858, seed=3, num_probes=8, dtype=torch.float32, device=DEV)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "last.pt")
    mp.spawn(_sharded_worker, args=(2, port, out), nprocs=2, join=True)
    got = torch.load(out)
    assert np.isclose(got["mean"].item(), mean.item(), rtol=2e-5)  # tests/test_gpu_sharded.py:170 (float32, f16x3: vtol 2e-5, gtol 5e-4)
    for a, b in zip(got["grads"], grads):
        assert torch.allclose(a, b.cpu(), rtol=5e-4, atol=5e-4 * b.abs().max().item()), (a, b)
