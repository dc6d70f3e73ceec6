"""Dense torch restatement of the random-feature prior paths and of Matheron's rule (any dtype, any device; the tests use fp64 as
the reference and fp32 on the CPU to size the fp32 bounds).  Nothing here calls libmfx."""

import math

import torch


def features(x, omega, phase, weights, lengthscale, outputscale):
    """(S, n): c sum_j cos(omega_j . x_i / l + b_j) W_sj, c = sqrt(2 outputscale / m)."""
    m = omega.shape[0]
    z = (x / lengthscale) @ omega.T + phase
    return math.sqrt(2.0 / m) * torch.sqrt(outputscale) * (weights @ torch.cos(z).T)


def phases(x, omega, phase, lengthscale):
    return (x / lengthscale) @ omega.T + phase


def kernel_matrix(kind, xa, xb, lengthscale, outputscale):
    """K(xa, xb) with the Gram operator's conventions (gp_util.kernel_scaled_*): eps of the dtype inside Matern's root."""
    a, b = xa / lengthscale, xb / lengthscale
    s = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    eps = torch.finfo(xa.dtype).eps
    if kind == "rbf":
        return outputscale * torch.exp(-s / 2)
    if kind == "matern12":
        return outputscale * torch.exp(-torch.sqrt(s + eps))
    if kind == "matern32":
        r = torch.sqrt(3 * s + eps)
        return outputscale * (1 + r) * torch.exp(-r)
    if kind == "matern52":
        r = torch.sqrt(5 * s + eps)
        return outputscale * (1 + r + r * r / 3) * torch.exp(-r)
    raise ValueError(kind)


def kernel_approx(xa, xb, omega, phase, lengthscale, outputscale):
    """c^2 sum_j cos(z_aj) cos(z_bj): the kernel the features represent."""
    m = omega.shape[0]
    ca, cb = torch.cos(phases(xa, omega, phase, lengthscale)), torch.cos(phases(xb, omega, phase, lengthscale))
    return 2.0 * outputscale / m * (ca @ cb.T)


def matheron(kind, X, y, mean, xs, omega, phase, weights, eps, lengthscale, outputscale, noise):
    """(S, len(xs)): mean + phi(xs) w_s + K(xs, X) (K + noise I)^-1 (y - mean - phi(X) w_s - eps_s), dense solve."""
    n = X.shape[0]
    A = kernel_matrix(kind, X, X, lengthscale, outputscale) + noise * torch.eye(n, dtype=X.dtype, device=X.device)
    rhs = (y - mean)[None, :] - features(X, omega, phase, weights, lengthscale, outputscale) - eps
    v = torch.linalg.solve(A, rhs.T).T
    return mean + features(xs, omega, phase, weights, lengthscale, outputscale) + v @ kernel_matrix(kind, xs, X, lengthscale, outputscale).T


def posterior_moments(kind, X, y, mean, xs, lengthscale, outputscale, noise):
    """(mean, variance) of the exact latent posterior at xs."""
    n = X.shape[0]
    A = kernel_matrix(kind, X, X, lengthscale, outputscale) + noise * torch.eye(n, dtype=X.dtype, device=X.device)
    Ks = kernel_matrix(kind, xs, X, lengthscale, outputscale)
    mu = mean + Ks @ torch.linalg.solve(A, y - mean)
    var = kernel_matrix(kind, xs, xs, lengthscale, outputscale).diagonal() - (Ks * torch.linalg.solve(A, Ks.T).T).sum(-1)
    return mu, var
