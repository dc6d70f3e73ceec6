"""NumPy restatement of modified batched CG as include/mfx.h specifies mfx_mbcg_solve: the PCG loop of cg.py with its safe division,
the recorded coefficients, the live-step rule, the padded Lanczos tridiagonal and the quadrature -- and the dense expressions they
are checked against.  Everything runs in the dtype of its inputs (float32 arrays give an fp32 run)."""

import numpy as np


def safe_div(a, b, eps2):
    """cg.py:222-241: a / b where |b| > eps^2, else a."""
    return a / b if (b > eps2 or b < -eps2) else a


def rbf_gram(X, lengthscale, outputscale, noise):
    """K(X, X) + noise I, k(x, y) = outputscale exp(-|x / l - y / l|^2 / 2), exact zeros on the diagonal's distance."""
    Xs = X / lengthscale
    sq = (Xs * Xs).sum(1)
    dist = np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xs @ Xs.T, 0.0)
    np.fill_diagonal(dist, 0.0)
    return outputscale * np.exp(-0.5 * dist) + noise * np.eye(len(X))


def pivoted_cholesky(K, rank):
    """low_rank.py:123-228 in the original row order: L (n, rank) with K ~ L L^T, pivot = largest residual diagonal."""
    n = K.shape[0]
    L = np.zeros((n, rank))
    for i in range(rank):
        d = np.diag(K) - (L[:, :i] ** 2).sum(1)
        piv = int(np.argmax(np.abs(d)))
        L[:, i] = (K[:, piv] - L[:, :i] @ L[piv, :i]) / np.sqrt(d[piv])
    return L


def woodbury(L, s, dtype):
    """v -> (s I + L L^T)^-1 v = (v - L (s I + L^T L)^-1 L^T v) / s, the small inverse formed in fp64 (low_rank.Preconditioner.minv)."""
    L64 = np.asarray(L, dtype=np.float64)
    minv = np.linalg.inv(L64.T @ L64 + s * np.eye(L.shape[1])).astype(dtype)
    Lt, s_t = np.asarray(L, dtype=dtype), dtype(s)
    return lambda v: ((v - Lt @ (minv @ (Lt.T @ v))) / s_t).astype(dtype)


def pcg(A, B, minv_apply, maxiter, adaptive=None):
    """PCG on every row of B (p, n): x = 0, r = b, z = M^-1 r, p = z; per step alpha = (r.z) / (p.Ap), beta = (r.z)' / (r.z).
    adaptive = (atol, rtol, miniter) or None (exactly maxiter steps).  -> x, r (p, n), num_steps (p), rz (p, maxiter + 1),
    pap (p, maxiter), w0 (p, n) = M^-1 b."""
    dtype = B.dtype.type
    eps2 = dtype(np.finfo(dtype).eps) ** 2
    nb, n = B.shape
    X, R, W0 = np.zeros_like(B), B.copy(), np.zeros_like(B)
    steps = np.zeros(nb, dtype=np.int64)
    rzs, paps = np.zeros((nb, maxiter + 1), dtype=dtype), np.zeros((nb, maxiter), dtype=dtype)
    precond = minv_apply if minv_apply is not None else (lambda v: v.copy())
    for b in range(nb):
        x, r = X[b], R[b]
        z = precond(r)
        W0[b] = z
        pv = z.copy()
        rz = dtype(r @ z)
        rzs[b, 0] = rz
        for it in range(maxiter):
            if adaptive is not None:
                atol, rtol, miniter = adaptive
                large = np.sqrt(np.mean((r / (dtype(atol) + np.abs(x) * dtype(rtol))) ** 2)) > 1.0
                if not (large or it < miniter):
                    break
            Ap = (A @ pv).astype(dtype)
            pap = dtype(pv @ Ap)
            paps[b, it] = pap
            alpha = safe_div(rz, pap, eps2)
            x += alpha * pv
            r -= alpha * Ap
            z = precond(r)
            rz_new = dtype(r @ z)
            beta = safe_div(rz_new, rz, eps2)
            pv = z + beta * pv
            rz = rz_new
            rzs[b, it + 1] = rz
            steps[b] += 1
    return X, R, steps, rzs, paps, W0


def tridiag(rzs, paps, steps, maxiter):
    """The padded Lanczos tridiagonal of M^-1/2 A M^-1/2 started at M^-1/2 b: with alpha_j = rz_j / pap_j, beta_j = rz_{j+1} / rz_j,
    tdiag[j] = 1 / alpha_j + beta_{j-1} / alpha_{j-1} (j < depth), toff[j] = sqrt(beta_j) / alpha_j (j < depth - 1), (1, 0) elsewhere.
    Step j is live when j < steps, rz_j > eps^2, pap_j > eps^2 and every earlier step is live; depth = the number of live steps."""
    dtype = rzs.dtype.type
    eps2 = dtype(np.finfo(dtype).eps) ** 2
    nb = rzs.shape[0]
    tdiag, toff = np.ones((nb, maxiter), dtype=dtype), np.zeros((nb, maxiter), dtype=dtype)
    depth = np.zeros(nb, dtype=np.int64)
    for b in range(nb):
        m = 0
        while m < min(steps[b], maxiter) and rzs[b, m] > eps2 and paps[b, m] > eps2:
            m += 1
        depth[b] = m
        for j in range(m):
            alpha = rzs[b, j] / paps[b, j]
            tdiag[b, j] = dtype(1) / alpha
            if j > 0:
                tdiag[b, j] += (rzs[b, j] / rzs[b, j - 1]) / (rzs[b, j - 1] / paps[b, j - 1])
            if j < m - 1:
                toff[b, j] = np.sqrt(rzs[b, j + 1] / rzs[b, j]) / alpha
    return tdiag, toff, depth


def quadrature(tdiag, toff, rz0):
    """rz0_b e1^T log(T_b) e1 per right-hand side, from a dense fp64 eigendecomposition of the padded tridiagonal."""
    out = np.zeros(len(rz0))
    for b in range(len(rz0)):
        k = tdiag.shape[1]
        T = np.diag(tdiag[b].astype(np.float64)) + np.diag(toff[b, : k - 1].astype(np.float64), 1) + np.diag(toff[b, : k - 1].astype(np.float64), -1)
        lam, U = np.linalg.eigh(T)
        out[b] = float(rz0[b]) * float((U[0] ** 2 * np.log(lam)).sum())
    return out


def _sym_fun(S, fun):
    lam, U = np.linalg.eigh(S)
    return (U * fun(lam)) @ U.T


def dense_quadform(A, M, Z):
    """z^T M^-1/2 log(M^-1/2 A M^-1/2) M^-1/2 z per row of Z, by dense fp64 eigendecompositions (M = None: the identity)."""
    A = np.asarray(A, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    if M is None:
        return np.einsum("bi,ij,bj->b", Z, _sym_fun(A, np.log), Z)
    Mih = _sym_fun(np.asarray(M, dtype=np.float64), lambda lam: 1.0 / np.sqrt(lam))
    inner = Mih @ A @ Mih
    logm = _sym_fun(0.5 * (inner + inner.T), np.log)
    V = Z @ Mih
    return np.einsum("bi,ij,bj->b", V, logm, V)


def table_setting(seed=0, n=96, d=3, noise=0.1, rank=8, probes=4):
    """The setting of the issue's table: RBF, n = 96, d = 3, noise 0.1, pivoted rank-8 factor of the noise-free kernel, 4 probes.
    -> X, (lengthscale, outputscale, noise), A (n, n), L (n, rank), M = noise I + L L^T, probes' raw signs R (probes, n + rank)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    lengthscale, outputscale = 1.0, 1.0
    A = rbf_gram(X, lengthscale, outputscale, noise)
    L = pivoted_cholesky(A - noise * np.eye(n), rank)
    M = noise * np.eye(n) + L @ L.T
    R = np.where(rng.random((probes, n + rank)) < 0.5, -1.0, 1.0)
    return X, (lengthscale, outputscale, noise), A, L, M, R


def probes_with_covariance(R, L, s):
    """sqrt(s) R[:, :n] + R[:, n:] L^T: covariance s I + L L^T for +-1 entries R."""
    n = L.shape[0]
    return np.sqrt(s) * R[:, :n] + R[:, n:] @ L.T
