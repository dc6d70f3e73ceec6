"""The diagonal and last-layer Laplace baselines of the reference's ``util/bnn_baselines.py`` -- MI355X build: what the full-GGN
calibration (``bnn_util.callibration_loss``) is compared against (``bnn_util.callibration_loss_diagonal``).

``exact_diagonal`` (:10-82) is one fused HIP pass over the tape of ``operators.GgnMlpOp`` (``mfx_ggn_diag``); ``hutchinson_diagonal``
(:108-165) is the reference's recursion over any batched matvec, the bound native operator included; ``last_layer_ggn`` (:169-204) is
plain torch on the same tape.  theta is the flat parameter vector in the layout of ``GgnMlpOp``.
"""

from __future__ import annotations

import torch

from ..operators import GgnMlpOp, _mlp_problem, _mlp_tape
from .bnn_util import _activation_name, _normal

_LIKELIHOODS = {"classification": "cross_entropy", "regression": "mse"}


def _loss_of(likelihood):
    if likelihood not in _LIKELIHOODS:
        raise ValueError(f"Argument likelihood = {likelihood} unknown.")
    return _LIKELIHOODS[likelihood]


def exact_diagonal(theta, x_train, widths, *, activation="tanh", likelihood="classification"):
    """util/bnn_baselines.py:10-82: sum_i diag(J_i^T H_i J_i), (P,), without a shift.  The reference takes N c^2 gradients (N c for
    regression); here it is ``GgnMlpOp(...).diagonal()``, c backward sweeps per sample in one kernel."""
    loss = _loss_of(likelihood)
    return GgnMlpOp(x_train, theta, widths, activation=_activation_name(activation), loss=loss).diagonal()


def hutchinson_diagonal(gvp_fn, like, n_samples, key, num_levels=5, computation_type="serial"):
    """util/bnn_baselines.py:108-165: Hutchinson's estimate of the diagonal of A with the running estimate as control variate.
    Within a level, with cv the diagonal of the earlier levels (0 at the first) and standard normal probes eps_b,

        update = mean_b[eps_b o (A eps_b - cv o eps_b)] + cv;      across levels   diag <- (diag n + update) / (n + 1),  n = 0, 1, ...

    ``gvp_fn`` is a bound native operator (``op.bind(alpha)``) or any batched callable (p, P) -> (p, P); ``like`` a (P,) tensor that
    fixes the size, dtype and device (the reference's ``params``).  "parallel" applies the ``n_samples`` probes of a level in one
    call, "serial" one at a time; both stack the products and evaluate the same expression, so for the same draws they differ only
    where ``gvp_fn`` itself depends on the batch (the native operators do not).  ``key``: an integer seed, or the draws themselves,
    (num_levels, n_samples, P)."""
    if computation_type not in ("serial", "parallel"):
        raise ValueError(f"computation_type must be 'serial' or 'parallel', got {computation_type!r}")
    n_samples, num_levels = int(n_samples), int(num_levels)
    if n_samples < 1 or num_levels < 1:
        raise ValueError("hutchinson_diagonal: n_samples and num_levels must be at least 1")
    P = like.numel()
    draws = _normal(key, (num_levels, n_samples, P), like.reshape(-1))
    if tuple(draws.shape) != (num_levels, n_samples, P):
        raise ValueError(f"hutchinson_diagonal: the draws must have shape {(num_levels, n_samples, P)}, got {tuple(draws.shape)}")
    diag = torch.zeros(P, dtype=draws.dtype, device=draws.device)
    for n in range(num_levels):
        eps = draws[n].contiguous()
        if computation_type == "parallel":
            gvp = gvp_fn(eps)
        else:
            gvp = torch.cat([gvp_fn(eps[b : b + 1]) for b in range(n_samples)])
        update = (eps * (gvp - diag * eps)).mean(0) + diag
        diag = (diag * n + update) / (n + 1)
    return diag.reshape(like.shape)


def last_layer_ggn(theta, x, widths, *, activation="tanh", likelihood="classification"):
    """util/bnn_baselines.py:169-204: the GGN block of the last layer's parameters, dense, ((w_{L-1} + 1) c)^2:

        sum_i (a~_i a~_i^T) (x) H_i,    a~ = [1, a_{L-1}],    H_i = diag(p_i) - p_i p_i^T (classification) or I (regression)

    rows and columns in theta's order (the bias, then the kernel row-major: index k~ c + m with k~ = 0 for the bias and k + 1 for
    input k).  It is the trailing block of ``bnn_util.ggn_full`` at alpha = 0.  (The reference's einsum for classification,
    "mob, boo, bon->mn", reads only the diagonal of H; this is the block of the GGN itself.)  Plain torch: it runs on any device."""
    loss = _loss_of(likelihood)
    widths, _, x2 = _mlp_problem("last_layer_ggn", x, theta, widths, _activation_name(activation), "x")
    tape = _mlp_tape(theta.detach(), x2, widths, _activation_name(activation), loss == "cross_entropy")
    a = tape["act"][-1]
    at = torch.cat([torch.ones_like(a[:, :1]), a], dim=1)  # (N, w + 1)
    c = widths[-1]
    if loss == "cross_entropy":
        p = tape["prob"]
        H = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
        G = torch.einsum("nk,nl,nab->kalb", at, at, H)
    else:
        G = torch.einsum("kl,ab->kalb", at.T @ at, torch.eye(c, dtype=at.dtype, device=at.device))
    n = at.shape[1] * c
    return G.reshape(n, n)
