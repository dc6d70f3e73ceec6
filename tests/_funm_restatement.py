"""torch-CPU fp64 restatement of f(A) v on the Lanczos path, written from the formulas of DESIGN.md section 3.5b (plain helper module).

    Q, alpha, beta = Krylov recurrence of depth k from v / |v|     (fully re-orthogonalised, or the three-term recurrence)
    lam, U = eigh(tridiag(alpha, beta));   c = U (f(lam) o U[0])
    y = |v| c^T Q

Everything is differentiable by autograd (through ``torch.linalg.eigh``: trustworthy for well separated Ritz values only, which is
why the device path has the divided-difference VJP that ``coeffs_vjp`` restates).  ``A`` is a dense symmetric matrix or a callable.
"""

import torch


def _apply(A, x):
    return A(x) if callable(A) else A @ x


def krylov_full(A, v, k):
    """Full re-orthogonalisation: every new vector is projected against the whole basis (twice), the projections of the first pass are
    column j of H = Q A Q^T, and the tridiagonal is the symmetric part of H.  v (n,) of unit length -> Q (k, n), alpha (k,), beta (k - 1,)."""
    rows, cols = [v], []
    for j in range(k):
        Q = torch.stack(rows)
        w = _apply(A, rows[j])
        h = Q @ w
        w = w - h @ Q
        w = w - (Q @ w) @ Q
        nrm = torch.linalg.vector_norm(w)
        cols.append(torch.cat([h, nrm[None], w.new_zeros(k)])[:k])
        if j + 1 < k:
            rows.append(w / nrm)
    H = torch.stack(cols, dim=1)
    T = 0.5 * (H + H.T)
    return torch.stack(rows), torch.diagonal(T), torch.diagonal(T, 1)


def krylov_three_term(A, v, k):
    """alpha_j = q_j^T A q_j,  beta_j q_{j+1} = A q_j - alpha_j q_j - beta_{j-1} q_{j-1}.  Same outputs as krylov_full."""
    rows, alpha, beta = [v], [], []
    for j in range(k):
        w = _apply(A, rows[j])
        a = rows[j] @ w
        w = w - a * rows[j]
        if j > 0:
            w = w - beta[j - 1] * rows[j - 1]
        alpha.append(a)
        if j + 1 < k:
            b = torch.linalg.vector_norm(w)
            beta.append(b)
            rows.append(w / b)
    return torch.stack(rows), torch.stack(alpha), torch.stack(beta) if beta else v.new_zeros(0)


def tridiag_matrix(alpha, beta):
    return torch.diag(alpha) + torch.diag(beta, 1) + torch.diag(beta, -1)


def coeffs(alpha, beta, f):
    """c = f(T) e1 = U (f(lam) o U[0])"""
    lam, U = torch.linalg.eigh(tridiag_matrix(alpha, beta))
    return U @ (f(lam) * U[0])


def funm(A, v, k, f, reortho="full"):
    """y = |v| c^T Q for one start vector v (n,)"""
    scale = torch.linalg.vector_norm(v)
    Q, alpha, beta = (krylov_full if reortho == "full" else krylov_three_term)(A, v / scale, k)
    return scale * (coeffs(alpha, beta, f) @ Q)


def funm_batched(A, V, k, f, reortho="full"):
    return torch.stack([funm(A, v, k, f, reortho) for v in V])


def divided_differences(lam, fl, dfl, rel_tol=1e-13):
    """F_ac = (f_a - f_c) / (lam_a - lam_c);  the mean of f' on the diagonal and wherever |lam_a - lam_c| <= rel_tol max|lam|"""
    dl = lam[:, None] - lam[None, :]
    same = (dl.abs() <= rel_tol * lam.abs().max()) | torch.eye(lam.numel(), dtype=torch.bool)
    mean = 0.5 * (dfl[:, None] + dfl[None, :])
    return torch.where(same, mean, (fl[:, None] - fl[None, :]) / torch.where(same, torch.ones_like(dl), dl))


def coeffs_vjp(lam, U, fl, dfl, dc, scale, rel_tol=1e-13):
    """Closed-form VJP of c = scale U (f(lam) o U[0]) w.r.t. the tridiagonal and the scale:
    w = U^T dc, M_ac = F_ac w_a U[0][c], G = U M U^T;  dalpha_i = scale G_ii, dbeta_i = scale (G_{i,i+1} + G_{i+1,i}), dscale = sum_a w_a f_a U[0][a]."""
    w = U.T @ dc
    M = divided_differences(lam, fl, dfl, rel_tol) * w[:, None] * U[0][None, :]
    G = U @ M @ U.T
    return scale * torch.diagonal(G), scale * (torch.diagonal(G, 1) + torch.diagonal(G, -1)), (w * fl * U[0]).sum()


def gram_matrix(X, raw_lengthscale, raw_outputscale, raw_noise, kernel="rbf", noise_minval=0.0):
    """K(X, X) + noise I of the project's scaled-kernel parametrisation (softplus of the raw values; include/mfx.h: MFX_KERNEL_*)."""
    sp = torch.nn.functional.softplus
    Z = X / sp(raw_lengthscale)
    s = ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(-1)
    if kernel == "rbf":
        K = torch.exp(-0.5 * s)
    elif kernel == "matern52":
        r = torch.sqrt(5.0 * s + torch.finfo(X.dtype).eps)
        K = (1.0 + r + r * r / 3.0) * torch.exp(-r)
    else:
        raise ValueError(kernel)
    return sp(raw_outputscale) * K + (noise_minval + sp(raw_noise)) * torch.eye(X.shape[0], dtype=X.dtype)
