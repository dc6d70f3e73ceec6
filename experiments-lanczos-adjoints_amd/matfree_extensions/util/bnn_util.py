"""The linearised-Laplace side of the reference's ``util/bnn_util.py`` -- MI355X build ("next" tier, §8f-3).

Samplers (:372-409): compositions of ``lanczos.tridiag(reortho="full")`` (the hot-path kernels) with a small dense factorisation of
the k x k tridiagonal matrix (torch, k <= ~100).

Calibration (:21-40, 43-61, 120-203, 218-228, 477-518): the reference's MLP on a flat parameter vector, the dense GGN baseline
(``ggn_full``, torch.func), the matrix-free GGN operator (``ggn_operator`` -> ``operators.GgnMlpOp``, one fused HIP pass over a tape
per matvec), the log-determinant solvers and the calibration losses.  The reference differentiates those losses in ``log_alpha``
alone, with theta and the data fixed; so does this module: a theta that requires grad is refused.

Predictive (:206-215, 549-683): N(f(x*; theta), J* (GGN + alpha I)^-1 J*^T) at test points -- the dense baseline ``predictive_cov``,
the matrix-free ``predictive_cov_operator`` (``operators.MlpJacobian`` for J* and J*^T, a batched CG on the bound GGN operator in
between), ``logpdf_cholesky`` / ``logpdf_eigh``, ``predictive_posterior_loglikelihood`` and ``predictive_logit_sampler``.

Diagonal baseline (:349-358, 433-474): ``ggn_diag`` (dense) and ``callibration_loss_diagonal`` on the Hutchinson or the exact diagonal
of the GGN; ``hutchinson_diagonal``, ``exact_diagonal`` and ``last_layer_ggn`` are in ``util/bnn_baselines.py``.

Conv nets, ViTs and data loaders are not here.
"""

from __future__ import annotations

import math

import torch

from .. import cg, hutchinson, lanczos
from ..operators import DenseOp, GgnMlpOp, MlpJacobian


def _normal(key, shape, like):
    if torch.is_tensor(key):
        return key  # explicit draws (the tests' way of fixing the randomness)
    gen = torch.Generator(device=like.device)
    gen.manual_seed(int(key))
    return torch.randn(shape, dtype=like.dtype, device=like.device, generator=gen)


def _dense_tridiag(diagonal, off_diagonal):
    """util/bnn_util.py:412-413 (batched)."""
    return torch.diag_embed(diagonal) + torch.diag_embed(off_diagonal, 1) + torch.diag_embed(off_diagonal, -1)


def sampler_cholesky(*, ggn_fun, num):
    """util/bnn_util.py:361-369: samples  variables + chol(ggn^{-1}) eps  (dense baseline)."""

    def sample(key, alpha, variables, x_train, y_train):
        ggn = ggn_fun(alpha, variables, x_train, y_train)
        ggn_inv_sqrt = torch.linalg.cholesky(torch.linalg.inv(ggn))
        eps = _normal(key, (num, *variables.shape), variables)
        return (ggn_inv_sqrt @ eps.T).T + variables[None, ...]

    return sample


def sampler_lanczos(*, ggn_fun, num, lanczos_rank):
    """util/bnn_util.py:372-389: per draw eps, Lanczos on the GGN started at eps, then  Q^T chol(T^{-1}) Q eps."""

    def sample(key, alpha, variables, x_train, y_train):
        ggn = ggn_fun(alpha, variables, x_train, y_train)
        tridiag = lanczos.tridiag(DenseOp().bind(ggn), lanczos_rank, reortho="full")
        eps = _normal(key, (num, *variables.shape), variables)
        (Q, (diag, off)), _ = tridiag(eps)  # Q (num, k, n)
        tri_inv_sqrt = torch.linalg.cholesky(torch.linalg.inv(_dense_tridiag(diag, off)))
        coeff = torch.einsum("bkn,bn->bk", Q, eps)
        return torch.einsum("bkn,bk->bn", Q, torch.einsum("bkl,bl->bk", tri_inv_sqrt, coeff)) + variables[None, ...]

    return sample


def lanczos_sampler(*, ggn_vp, num_samples, lanczos_rank, key, params_vec):
    """util/bnn_util.py:392-409: eigen-decomposition of the Lanczos tridiagonal matrix, eigenvalues below 1e-9 dropped."""
    eps = _normal(key, (num_samples, *params_vec.shape), params_vec)
    (Q, (diag, off)), _ = lanczos.tridiag(ggn_vp, lanczos_rank, reortho="full")(eps)
    w, v = torch.linalg.eigh(_dense_tridiag(diag, off))
    eigvecs = Q.transpose(-1, -2) @ v  # (num, n, k)
    small = w < 1e-9
    inv_eigvals = torch.where(small, torch.zeros_like(w), 1 / torch.where(small, torch.ones_like(w), w))
    sample = torch.sqrt(inv_eigvals) * eps[:, :lanczos_rank]
    return params_vec + torch.einsum("bnk,bk->bn", eigvecs, sample)


# ------------------------------------------------------------------------------------------------
# the reference's MLP on a flat parameter vector (util/bnn_util.py:21-40, 502-518)
# ------------------------------------------------------------------------------------------------
_HIDDEN = (50, 50, 5, 5)
_ACTIVATIONS = {"tanh": torch.tanh, "relu": torch.relu}


def _activation_name(activation):
    if activation in _ACTIVATIONS:
        return activation
    for name, fn in _ACTIVATIONS.items():
        if activation is fn:
            return name
    raise ValueError("activation must be 'tanh' or 'relu' (or torch.tanh / torch.relu)")


def mlp_unflatten(theta, widths):
    """flat theta -> [{"bias": (w_l,), "kernel": (w_{l-1}, w_l)}, ...]: per layer the bias, then the kernel row-major -- the order of
    flax's ravel_pytree for the reference's model (Dense_0.bias, Dense_0.kernel, Dense_1.bias, ...)."""
    out, off = [], 0
    for wi, wo in zip(widths[:-1], widths[1:]):
        out.append({"bias": theta[off : off + wo], "kernel": theta[off + wo : off + wo + wi * wo].reshape(wi, wo)})
        off += (wi + 1) * wo
    if off != theta.numel():
        raise ValueError(f"widths {tuple(widths)} have {off} parameters, theta has {theta.numel()}")
    return out


def mlp_apply(theta, x, widths, activation="tanh"):
    """logits of the MLP with flat parameters ``theta`` (plain torch ops: differentiable, torch.func-transformable)"""
    phi = _ACTIVATIONS[_activation_name(activation)]
    a = x.reshape(x.shape[0], -1)
    layers = mlp_unflatten(theta, widths)
    for l, layer in enumerate(layers):
        a = a @ layer["kernel"] + layer["bias"]
        if l + 1 < len(layers):
            a = phi(a)
    return a


def model_mlp(*, out_dims, activation="tanh"):
    """util/bnn_util.py:21-40: Dense(50), Dense(50), Dense(5), Dense(5), Dense(out_dims) with ``activation`` between them.
    Returns (init, apply) on the FLAT theta: ``init(key, x)`` -> theta (kernels LeCun-normal, biases zero, flax's defaults) for
    widths ``init.widths(d_in) = (d_in, 50, 50, 5, 5, out_dims)``; ``apply(theta, x)`` -> logits."""
    name = _activation_name(activation)

    def widths(d_in):
        return (int(d_in), *_HIDDEN, int(out_dims))

    def init(key, x):
        w = widths(x.reshape(x.shape[0], -1).shape[1])
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(key))
        parts = []
        for wi, wo in zip(w[:-1], w[1:]):
            parts += [torch.zeros(wo, dtype=torch.float64), (torch.randn(wi, wo, generator=gen, dtype=torch.float64) / math.sqrt(wi)).reshape(-1)]
        return torch.cat(parts).to(dtype=x.dtype, device=x.device)

    def apply(theta, x):
        return mlp_apply(theta, x, widths(x.reshape(x.shape[0], -1).shape[1]), name)

    init.widths = apply.widths = widths
    apply.activation = name
    return init, apply


def vectorize_nn(model_fn, params):
    """util/bnn_util.py:502-518 for the parameter trees of this module (a list of {"bias", "kernel"} per layer):
    -> (params_vec, unflatten_fn, model_apply_vec)."""
    shapes = [tuple(layer["kernel"].shape) for layer in params]
    widths = (shapes[0][0], *(s[1] for s in shapes))
    params_vec = torch.cat([t.reshape(-1) for layer in params for t in (layer["bias"], layer["kernel"])])

    def unflatten_fn(vec):
        return mlp_unflatten(vec, widths)

    def model_apply_vec(params_vectorized, x):
        return model_fn(unflatten_fn(params_vectorized), x)

    return params_vec, unflatten_fn, model_apply_vec


# ------------------------------------------------------------------------------------------------
# metrics and losses (util/bnn_util.py:43-61, 106-114)
# ------------------------------------------------------------------------------------------------
def metric_accuracy(*, probs, labels_hot):
    assert probs.dim() == 2 and labels_hot.dim() == 2
    return (probs.argmax(-1) == labels_hot.argmax(-1)).to(probs.dtype).mean(-1)


def metric_nll(*, logits, labels_hot, sum_or_mean_fun=torch.sum):
    assert logits.dim() == 2 and labels_hot.dim() == 2
    nll = (labels_hot * torch.log_softmax(logits, -1)).sum(-1)
    return -sum_or_mean_fun(nll, 0)


def metric_confidence(*, probs):
    assert probs.dim() == 2
    return probs.max(-1).values.mean(0)


def loss_training_cross_entropy_single(logits, labels_hot):
    return -(torch.log_softmax(logits, -1) * labels_hot).sum(-1)


def loss_training_mse_single(pred, target):
    """0.5 |pred - target|^2: logit Hessian = I (the "mse" loss of GgnMlpOp)"""
    return 0.5 * ((pred - target) ** 2).sum(-1)


# ------------------------------------------------------------------------------------------------
# the GGN: dense baseline and matrix-free operator (util/bnn_util.py:218-228, 263-293)
# ------------------------------------------------------------------------------------------------
def ggn_full(*, loss_single, model_fun, param_unflatten):
    """util/bnn_util.py:218-228: sum_i J_i^T H_i J_i + alpha I as a dense matrix (torch.func; the baseline the operator is tested against)"""

    def ggn_fun(alpha, variables, x_train, y_train):
        def f(v):
            return model_fun(param_unflatten(v), x_train)

        H = torch.func.vmap(torch.func.hessian(loss_single, argnums=0))(f(variables), y_train)
        J = torch.func.jacrev(f)(variables)  # (N, c, P)
        ggn = torch.einsum("nci,ncd,ndj->ij", J, H, J)
        return ggn + alpha * torch.eye(J.shape[-1], dtype=J.dtype, device=J.device)

    return ggn_fun


def ggn_diag(*, loss_single, model_fun, param_unflatten):
    """util/bnn_util.py:349-358, the dense diagonal baseline: diag(diag(ggn_full)), the shift included as in the reference"""
    ggn_fun_full = ggn_full(loss_single=loss_single, model_fun=model_fun, param_unflatten=param_unflatten)

    def ggn_fun(alpha, variables, x_train, y_train):
        return torch.diag(torch.diagonal(ggn_fun_full(alpha, variables, x_train, y_train)))

    return ggn_fun


def ggn_operator(theta, x_train, widths, *, activation="tanh", loss="cross_entropy"):
    """The matrix-free counterpart of ``ggn_full`` for an MLP: ``op(v, alpha)`` = (sum_i J_i^T H_i J_i + alpha I) v as one fused HIP
    pass over a tape built once here (theta and x_train fixed; with one-hot labels the labels do not enter either Hessian)."""
    return GgnMlpOp(x_train, theta, widths, activation=_activation_name(activation), loss=loss)


# ------------------------------------------------------------------------------------------------
# log-determinants and the calibration losses (util/bnn_util.py:120-203, 477-499)
# ------------------------------------------------------------------------------------------------
def solver_logdet_dense():
    def logdet(M):
        return torch.linalg.slogdet(M)[1]

    return logdet


def slq_log_clipped(*, clip_value=1.0):
    def log(x):
        eps = torch.finfo(x.dtype).eps
        return torch.log(torch.where(x < eps, torch.full_like(x, clip_value), x))

    return log


def _slq_mean(integrand, sampler, key, slq_num_batches, *args):
    estimate = hutchinson.hutchinson(integrand, sampler)
    if torch.is_tensor(key):  # explicit probes: one batch
        return estimate(key, *args)
    values = torch.stack([estimate(k, *args) for k in hutchinson.split(key, slq_num_batches)])
    return values.mean(0)


def solver_logdet_slq(*, lanczos_rank, slq_num_samples, slq_num_batches):
    """util/bnn_util.py:173-186: SLQ on a dense matrix M (the clipped log as matrix function)"""

    def logdet(M, key):
        sampler = hutchinson.sampler_rademacher(M[0], num=slq_num_samples)
        integrand = lanczos.integrand_spd(slq_log_clipped(), lanczos_rank, DenseOp().bind(M))
        return _slq_mean(integrand, sampler, key, slq_num_batches)

    return logdet


def solver_logdet_slq_implicit(*, lanczos_rank, slq_num_samples, slq_num_batches, N, x_like=None):
    """util/bnn_util.py:189-203: SLQ on a matvec ``Av(v, *args)`` (a native operator, or any callable).  ``key``: an integer seed, or
    the (slq_num_samples, N) probes themselves; ``x_like`` fixes dtype and device of generated probes (default: float32 on cuda)."""

    def logdet(Av, key, *args):
        like = key[0] if torch.is_tensor(key) else (x_like if x_like is not None else torch.ones(N, device="cuda"))[:N]
        sampler = hutchinson.sampler_rademacher(like, num=slq_num_samples)
        integrand = lanczos.integrand_spd(torch.log, lanczos_rank, Av)
        return _slq_mean(integrand, sampler, key, slq_num_batches, *args)

    return logdet


def loss_calibration(*, ggn_fun, hyperparam_unconstrain, logdet_fun):
    """util/bnn_util.py:120-135.  ``ggn_fun(alpha, variables, x_train, y_train)`` returns whatever ``logdet_fun`` takes: a dense matrix
    (``ggn_full`` with ``solver_logdet_dense`` / ``solver_logdet_slq``) or a bound operator (``ggn_operator(...).bind(alpha)``)."""

    def loss(a, variables, x_train, y_train, *logdet_params):
        alpha = hyperparam_unconstrain(a)
        log_prior = len(variables) / 2 * torch.log(alpha) - 0.5 * alpha * torch.dot(variables, variables)
        M = ggn_fun(alpha, variables, x_train, y_train)
        return -(log_prior - 0.5 * logdet_fun(M, *logdet_params))

    return loss


def callibration_loss(model_apply, unflatten, hyperparam_unconstrain, n_params, *, loss="cross_entropy", operator=None):
    """util/bnn_util.py:477-499 (the reference's spelling): SLQ with Lanczos rank 10 and 10 probes on the matrix-free GGN + alpha I.
    ``model_apply`` is ``model_mlp``'s apply (it names the widths and the activation; ``unflatten`` is unused: theta stays flat).
    ``loss(log_alpha, params_vec, img, label, key)`` is differentiable in ``log_alpha`` only.  The operator (and its tape) is kept
    while the SAME two tensor objects come back (the cache holds them, so their identity cannot be reused by other tensors; tensors
    modified in place between calls are the caller's to avoid) and rebuilt otherwise; ``operator=`` fixes what is applied instead (``lambda tape_op, alpha: bound matvec`` --
    the tests put a DenseOp of the same matrix there)."""
    cache = {}

    def loss_fn(log_alpha, params_vec, img, label, key):
        if params_vec.requires_grad or img.requires_grad:
            raise NotImplementedError("callibration_loss differentiates log_alpha only: theta and the data are fixed (their gradients "
                                      "need third derivatives of the network, which the reference never takes)")
        alpha = hyperparam_unconstrain(log_alpha)
        if cache.get("theta") is not params_vec or cache.get("img") is not img:
            d_in = img.reshape(img.shape[0], -1).shape[1]
            cache["theta"], cache["img"] = params_vec, img
            cache["op"] = ggn_operator(params_vec, img, model_apply.widths(d_in), activation=model_apply.activation, loss=loss)
        op = cache["op"]
        bound = op.bind(alpha) if operator is None else operator(op, alpha)
        logdet_fun = solver_logdet_slq_implicit(lanczos_rank=10, slq_num_samples=10, slq_num_batches=1, N=n_params, x_like=params_vec)
        logdet = logdet_fun(bound, key)
        log_prior = torch.log(alpha) * n_params - alpha * torch.dot(params_vec, params_vec)
        return -(log_prior - logdet)

    return loss_fn


def callibration_loss_diagonal(model_apply, unflatten, hyperparam_unconstrain, hutchinson_samples, num_levels, n_params, *,
                               loss="cross_entropy", exact=False, key=0, operator=None):
    """util/bnn_util.py:433-474, the diagonal-Laplace counterpart of ``callibration_loss``:

        -(log(alpha) n_params - alpha |theta|^2 - sum log(diag + alpha)),     entries of diag below 1e-4 set to 0

    with diag the diagonal of the GGN WITHOUT the shift: ``bnn_baselines.hutchinson_diagonal`` ("serial", ``hutchinson_samples``
    probes on each of ``num_levels`` levels; ``key`` an integer seed -- the reference fixes PRNGKey(0) -- or the draws themselves,
    (num_levels, hutchinson_samples, n_params)) over the operator bound to the shift 0, or, ``exact=True``, ``op.diagonal()`` (what
    the reference keeps commented out: N c^2 gradients there, one kernel here).  ``loss(log_alpha, params_vec, img, label)`` is
    differentiable in ``log_alpha`` only, through the explicit ``+ alpha``: the diagonal is a constant.  ``model_apply``,
    ``unflatten`` and the cache of the operator as in ``callibration_loss`` (the diagonal is kept with the operator: it does not
    depend on alpha); ``operator=`` fixes what the probes are applied to (``lambda tape_op, zero: batched matvec``)."""
    from .bnn_baselines import hutchinson_diagonal  # (bnn_baselines imports this module)

    cache = {}

    def loss_fn(log_alpha, params_vec, img, label):
        if params_vec.requires_grad or img.requires_grad:
            raise NotImplementedError("callibration_loss_diagonal differentiates log_alpha only: theta and the data are fixed (their "
                                      "gradients need third derivatives of the network, which the reference never takes)")
        alpha = hyperparam_unconstrain(log_alpha)
        if cache.get("theta") is not params_vec or cache.get("img") is not img:
            d_in = img.reshape(img.shape[0], -1).shape[1]
            cache["theta"], cache["img"] = params_vec, img
            op = ggn_operator(params_vec, img, model_apply.widths(d_in), activation=model_apply.activation, loss=loss)
            with torch.no_grad():
                if exact:
                    diag = op.diagonal()
                else:
                    zero = torch.zeros((), dtype=params_vec.dtype, device=params_vec.device)  # the shift stays out of the estimate
                    bound = op.bind(zero) if operator is None else operator(op, zero)
                    diag = hutchinson_diagonal(bound, params_vec, hutchinson_samples, key, num_levels=num_levels,
                                               computation_type="serial")
            cache["op"], cache["diag"] = op, diag
        diag = cache["diag"]
        diag = torch.where(diag < 1e-4, torch.zeros_like(diag), diag)
        logdet = torch.log(diag + alpha).sum()
        log_prior = torch.log(alpha) * n_params - alpha * torch.dot(params_vec, params_vec)
        return -(log_prior - logdet)

    return loss_fn


# ------------------------------------------------------------------------------------------------
# the predictive distribution at test points (util/bnn_util.py:206-215, 549-683)
# ------------------------------------------------------------------------------------------------
_REFERENCE_CG_STEPS = 20  # krylov_solve_cg_fixed_step_reortho(20), hard-coded at util/bnn_util.py:643, 668


def _cov_matrix(cov, mean):
    """``cov`` applied to the identity in ONE batched call (the reference: jacfwd / jacfwd_map of cov at the mean, column by
    column): row b of the result of the call is cov e_b, the b-th column of the matrix."""
    n = mean.shape[0]
    return cov(torch.eye(n, dtype=mean.dtype, device=mean.device)).T


def logpdf_cholesky():
    """util/bnn_util.py:549-574: ``logpdf(y, mean=, cov=)`` -> (value, {}) of N(mean, C) by a Cholesky factorisation; ``cov`` is a
    callable that applies C to a batch of vectors, (p, n) -> (p, n)."""

    def logpdf(y, /, *, mean, cov):
        cholesky = torch.linalg.cholesky(_cov_matrix(cov, mean))
        logdet = torch.log(torch.diagonal(cholesky)).sum()
        tmp = torch.linalg.solve_triangular(cholesky, (y - mean)[:, None], upper=False)[:, 0]
        mahalanobis = torch.dot(tmp, tmp)
        (n,) = mean.shape
        return -logdet - 0.5 * mahalanobis - n / 2 * math.log(2 * math.pi), {}

    return logpdf


def _eigh(cov_matrix):
    """jnp.linalg.eigh symmetrises its input by default; torch reads one triangle, so the mean of both is taken here"""
    return torch.linalg.eigh(0.5 * (cov_matrix + cov_matrix.T))


def logpdf_eigh():
    """util/bnn_util.py:599-627: the same by a symmetric eigendecomposition, with the reference's rules as written: an eigenvalue
    below 1e-6 counts as 1 in the log-determinant and as 0 (not 1 / w) in the Mahalanobis norm."""

    def logpdf(y, /, *, mean, cov):
        w, v = _eigh(_cov_matrix(cov, mean))
        small = w < 1e-6
        logdet = torch.log(torch.where(small, torch.ones_like(w), w)).sum() / 2
        inv_eigvals = torch.where(small, torch.zeros_like(w), 1 / torch.where(small, torch.ones_like(w), w))
        factor = (v * torch.sqrt(inv_eigvals)[None, :]) @ v.T
        tmp = factor @ (y - mean)
        mahalanobis = torch.dot(tmp, tmp)
        (n,) = mean.shape
        return -logdet - 0.5 * mahalanobis - n / 2 * math.log(2 * math.pi), {}

    return logpdf


def predictive_cov(*, ggn_fun, model_fun, param_unflatten, hyperparam_unconstrain):
    """util/bnn_util.py:206-215, the dense baseline: the inverse of the full GGN (``ggn_full``) and the test Jacobian by
    torch.func.jacrev; ``evaluate(a, variables, x_train, y_train, x_test)`` -> (N*, c, c), J_i (GGN + alpha I)^-1 J_i^T per point."""

    def evaluate(a, variables, x_train, y_train, x_test):
        alpha = hyperparam_unconstrain(a)
        covariance = torch.linalg.inv(ggn_fun(alpha, variables, x_train, y_train))
        J_test = torch.func.jacrev(lambda v: model_fun(param_unflatten(v), x_test))(variables)  # (N*, c, P)
        return torch.einsum("nci,ij,ndj->ncd", J_test, covariance, J_test)

    return evaluate


def predictive_cov_operator(ggn_op, jac, *, solve=None, chunk=32):
    """The same per-point covariances without a matrix: ``ggn_op`` is a ``GgnMlpOp`` over the training set (anything with
    ``bind(alpha)``), ``jac`` an ``operators.MlpJacobian`` over the test points (anything with ``rows`` / ``apply`` / ``t_apply`` /
    ``n_samples`` / ``n_out``), ``solve(A, B) -> (X, info)`` a batched solver of ``cg.*`` (default: ``cg.cg_fixed_step_reortho(20)``,
    what the reference hard-codes).  ``evaluate(alpha)`` -> (N*, c, c).  Per chunk of B <= ``chunk`` test points: R = J_c^T I
    (B c unit cotangents -> (B c, P)), S = solve(ggn_op.bind(alpha), R), C = J_c S, of which the B diagonal c x c blocks are kept.
    Memory per chunk: three (B c, P) matrices and the solver's own."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"predictive_cov_operator: chunk must be >= 1, got {chunk}")
    solve = cg.cg_fixed_step_reortho(_REFERENCE_CG_STEPS) if solve is None else solve

    def evaluate(alpha):
        bound = ggn_op.bind(alpha)
        n, c = jac.n_samples, jac.n_out
        blocks = []
        for i0 in range(0, n, chunk):
            part = jac.rows(i0, min(i0 + chunk, n))
            B = part.n_samples
            eye = torch.eye(B * c, dtype=part.logits.dtype, device=part.logits.device)
            R = part.t_apply(eye.reshape(B * c, B, c))
            S, _info = solve(bound, R)
            C = part.apply(S).reshape(B, c, B, c)  # C[a, j, a', k] = (J_a' A^-1 J_a^T)[k, j]
            idx = torch.arange(B, device=C.device)
            blocks.append(C[idx, :, idx, :].transpose(-1, -2))
        return torch.cat(blocks)

    return evaluate


def _mlp_jacobian(model_apply):
    """(params_vec, x_test) -> MlpJacobian for ``model_mlp``'s apply, which names the widths and the activation"""

    def jacobian(params_vec, x_test):
        d_in = x_test.reshape(x_test.shape[0], -1).shape[1]
        return MlpJacobian(x_test, params_vec, model_apply.widths(d_in), activation=model_apply.activation)

    return jacobian


def _joint_cov_vp(jac, ggn_fun, solve):
    """v -> J* solve(ggn_fun, J*^T v) on batches (p, N* c) of flattened logit vectors: the joint (N* c)^2 predictive covariance"""
    n, c = jac.n_samples, jac.n_out

    def cov_vp(V):
        R = jac.t_apply(V.reshape(V.shape[0], n, c))
        S, _info = solve(ggn_fun, R)
        return jac.apply(S).reshape(V.shape[0], n * c)

    return cov_vp


def predictive_posterior_loglikelihood(*, model_apply, unflatten, logpdf, ggn_fun, solve=None, jacobian=None):
    """util/bnn_util.py:630-652: ``eval_logprob(params_vec, x_test, y_test)`` -> ``logpdf(y, mean=f(x*), cov=J* solve(ggn_fun, J*^T .))``
    over the flattened logits.  ``model_apply`` is ``model_mlp``'s apply (it names the widths and the activation; ``unflatten`` is
    unused: theta stays flat); ``ggn_fun`` a bound operator (``ggn_operator(...).bind(alpha)``) or any callable v -> A v;
    ``solve`` defaults to the reference's ``cg.cg_fixed_step_reortho(20)``.  ``jacobian=`` fixes what stands for J* instead
    (``lambda params_vec, x_test: object with logits / apply / t_apply`` -- the tests put a dense Jacobian there)."""
    solve = cg.cg_fixed_step_reortho(_REFERENCE_CG_STEPS) if solve is None else solve
    jacobian = _mlp_jacobian(model_apply) if jacobian is None else jacobian

    def eval_logprob(params_vec, x_test, y_test):
        jac = jacobian(params_vec, x_test)
        return logpdf(y_test.reshape(-1), mean=jac.logits.reshape(-1), cov=_joint_cov_vp(jac, ggn_fun, solve))

    return eval_logprob


def predictive_logit_sampler(*, model_apply, unflatten, num_samples, ggn_fun, solve=None, jacobian=None):
    """util/bnn_util.py:655-683: ``eval_test_set(params_vec, x_test, y_test, key)`` -> (num_samples, *y_test.shape) logit samples
    mean + F eps with F = V diag(sqrt(1 / w)) V^T from the eigendecomposition of the joint covariance.  A quirk of the reference,
    reproduced: the root is taken of 1 / w (0 where w < 1e-6), so F is the inverse square root of the covariance, not its square
    root.  ``key``: an integer seed, or the (num_samples, N* c) draws ``eps`` themselves.  The other arguments as in
    ``predictive_posterior_loglikelihood``."""
    solve = cg.cg_fixed_step_reortho(_REFERENCE_CG_STEPS) if solve is None else solve
    jacobian = _mlp_jacobian(model_apply) if jacobian is None else jacobian

    def eval_test_set(params_vec, x_test, y_test, key):
        jac = jacobian(params_vec, x_test)
        mean = jac.logits.reshape(-1)
        w, v = _eigh(_cov_matrix(_joint_cov_vp(jac, ggn_fun, solve), mean))
        small = w < 1e-6
        inv_eigvals = torch.where(small, torch.zeros_like(w), 1 / torch.where(small, torch.ones_like(w), w))
        cov_sqrt = (v * torch.sqrt(inv_eigvals)[None, :]) @ v.T
        eps = _normal(key, (num_samples, mean.shape[0]), mean)
        return (mean[None, :] + eps @ cov_sqrt.T).reshape(num_samples, *y_test.shape)

    return eval_test_set
