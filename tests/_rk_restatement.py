"""fp64 torch restatement of the fixed-step explicit Runge-Kutta solves of y' = A y on a DENSE matrix: the yardstick of
tests/test_rk_host.py and tests/test_gpu_rk.py.

  solve      the generic explicit-RK loop; torch autograd through it is the discrete adjoint (discretise-then-differentiate)
  backsolve  the continuous adjoint written out: the same tableau integrated backwards from t1 with steps h = -dt on
             y' = A y, lam' = -A^T lam, Abar' = -lam y^T, the quadrature of a step being sum_i (-h b_i) Lam_i Y_i^T over the stages

States are rows: y (p, n), one step computes K_i = Y_i A^T.  The dense forms of the operators under test are here too: the ragged
CSR matrix (tests/_ragged_csr.py) and the stencil systems (tests/_stencil_restatement.py), with the maps from a dense cotangent
of A back to the operator's own parameters."""

import numpy as np
import torch

import _ragged_csr as rc
import _stencil_restatement as sr


def full_tableau(tab):
    """(a (s, s) strictly lower, b (s,)) as fp64 tensors from a rk_tableaux.Tableau"""
    s = len(tab.b)
    a = torch.zeros((s, s), dtype=torch.float64)
    for i, row in enumerate(tab.a):
        for j, v in enumerate(row):
            a[i, j] = float(v)
    return a, torch.tensor([float(v) for v in tab.b], dtype=torch.float64)


def step(A, y, a, b, h):
    """one step of size h -> (y+, [Y_i], [K_i]); A: a dense matrix, or a callable Y -> K on rows (the matrix-free stencil below)"""
    apply = A if callable(A) else (lambda Y: Y @ A.T)
    Ys, Ks = [], []
    for i in range(len(b)):
        Y = y
        for j in range(i):
            if float(a[i, j]) != 0.0:
                Y = Y + (h * a[i, j]) * Ks[j]
        Ys.append(Y)
        Ks.append(apply(Y))
    out = y
    for i in range(len(b)):
        if float(b[i]) != 0.0:
            out = out + (h * b[i]) * Ks[i]
    return out, Ys, Ks


def solve(A, y0, tab, dts, return_ys=False):
    a, b = full_tableau(tab)
    y, ys = y0, [y0]
    for dt in dts:
        y, _, _ = step(A, y, a, b, float(dt))
        ys.append(y)
    return (y, torch.stack(ys, dim=1)) if return_ys else y


def discrete_gradients(A, y0, tab, dts, dy1):
    """autograd through the loop -> (y1, dy0, dA)"""
    A = A.detach().clone().requires_grad_(True)
    y0 = y0.detach().clone().requires_grad_(True)
    y1 = solve(A, y0, tab, dts)
    dy0, dA = torch.autograd.grad(y1, (y0, A), dy1)
    return y1.detach(), dy0, dA


def backsolve(A, y1, dy1, tab, dts):
    """the continuous adjoint, discretised with the same tableau -> (dy0, dA)"""
    a, b = full_tableau(tab)
    y, lam = y1.clone(), dy1.clone()
    dA = torch.zeros_like(A)
    for dt in reversed([float(d) for d in dts]):
        h = -dt
        ynew, Ys, _ = step(A, y, a, b, h)
        # lam' = -A^T lam: the field of lam (rows) is -lam A
        lnew, Ls, _ = step(-A.T, lam, a, b, h)
        for i in range(len(b)):
            dA = dA + (-h * b[i]) * (Ls[i].T @ Ys[i])
        y, lam = ynew, lnew
    return lam, dA


# ---- dense forms of the operators under test ---------------------------------------------------------------------------------
def csr_case(n, seed):
    """(row, col, vals scaled so that |A|_inf <= 1, dense A) of a ragged CSR matrix"""
    rng = np.random.default_rng(seed)
    row, col, vals = rc.ragged_csr(n, rng)
    A = rc.dense_of(row, col, vals, n)
    scale = 1.0 / np.abs(A).sum(1).max()
    return row, col, vals * scale, A * scale


def csr_gradient(dA, row, col):
    """the cotangent of the stored values from a dense cotangent of A"""
    return dA[row, col]


def stencil_case(form, stencil, boundary, coef, ny, nx):
    return sr.cached_matrices(form, np.asarray(stencil, dtype=np.float64), boundary, coef, ny, nx)[0]


def stencil_gradient(form, stencil, boundary, dA, ny, nx):
    return sr.contract_dense_gradient(form, np.asarray(stencil, dtype=np.float64), boundary, dA, ny, nx)


# ---- the same two gradients for an operator given as a function of its parameter, without its matrix --------------------------
# For the one grid of tests/test_gpu_rk.py whose dense matrix (8580 x 8580) is too large to assemble in a test of seconds.
# tests/test_rk_host.py holds these against the dense forms above at a grid where both exist.
def torch_stencil_apply(form, stencil, boundary, ny, nx):
    """apply(Y, coef) on rows Y (p, n), written from util/pde_util.py:74-157 with torch pads and slices (fp64, differentiable)"""
    w = torch.tensor(np.asarray(stencil, dtype=np.float64))

    def conv(u):  # (p, ny, nx): convolve2d(stencil, padded, "valid")
        if boundary == "neumann":
            up = torch.nn.functional.pad(u[:, None], (1, 1, 1, 1), mode="replicate")[:, 0]
        else:
            up = torch.nn.functional.pad(u, (1, 1, 1, 1))
        out = torch.zeros_like(u)
        for a_ in range(3):
            for b_ in range(3):
                out = out + w[a_, b_] * up[:, 2 - a_ : 2 - a_ + ny, 2 - b_ : 2 - b_ + nx]
        return out

    def apply(Y, coef):
        p, m = Y.shape[0], ny * nx
        fx = (coef.reshape(1, ny, nx) * conv(Y[:, :m].reshape(p, ny, nx))).reshape(p, m)
        if form == "heat":
            return fx
        return torch.cat([-fx, Y[:, m:]], 1) if form == "heat2" else torch.cat([Y[:, m:], fx], 1)

    return apply


def discrete_gradients_fn(apply, theta, y0, tab, dts, dy1):
    """autograd through the loop with K = apply(Y, theta) -> (y1, dy0, dtheta)"""
    theta = theta.detach().clone().requires_grad_(True)
    y0 = y0.detach().clone().requires_grad_(True)
    y1 = solve(lambda Y: apply(Y, theta), y0, tab, dts)
    dy0, dth = torch.autograd.grad(y1, (y0, theta), dy1)
    return y1.detach(), dy0, dth


def backsolve_fn(apply, theta, y1, dy1, tab, dts):
    """the backsolve recursion with A^T L and the quadrature term taken from the bilinear form <L, apply(Y, theta)>"""
    a, b = full_tableau(tab)
    theta = theta.detach().clone().requires_grad_(True)

    def minus_transpose(L):  # rows of -(A^T L)
        Yd = torch.zeros_like(L, requires_grad=True)
        (g,) = torch.autograd.grad(apply(Yd, theta), Yd, L)
        return -g

    y, lam = y1.clone(), dy1.clone()
    dth = torch.zeros_like(theta)
    for dt in reversed([float(d) for d in dts]):
        h = -dt
        ynew, Ys, _ = step(lambda Y: apply(Y, theta).detach(), y, a, b, h)
        lnew, Ls, _ = step(minus_transpose, lam, a, b, h)
        for i in range(len(b)):
            if float(b[i]) != 0.0:
                (g,) = torch.autograd.grad((Ls[i] * apply(Ys[i], theta)).sum(), theta)
                dth = dth + (-h * b[i]) * g
        y, lam = ynew, lnew
    return lam, dth
