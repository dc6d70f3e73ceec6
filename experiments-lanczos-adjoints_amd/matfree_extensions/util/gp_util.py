"""Gaussian-process helpers on the SLQ log-determinant path -- MI355X build.

Covers the pieces of the reference's ``util/gp_util.py`` that sit on the hot path: the scaled-RBF
kernel parametrisation (:151-184), the softplus constraint (:187-201), the Gram matvec (:434-549,
here a native matrix-free operator instead of materialised row partitions) and the SLQ log-determinant
estimators (:552-621); plus the "next" tier: the model / likelihood / logpdf plumbing of the
log-marginal likelihood and of the posterior mean (:15-66, 216-351, 367-431) on top of ``cg`` and ``low_rank``.
"""

from __future__ import annotations

import torch

import ctypes as C
import math

from .. import _lib, cg, hutchinson, lanczos, low_rank
from ..operators import (BoundOp, CallbackOp, NativeOp, PreconditionedOp, RandomFeatures, RbfGramOp, RowShardedOp, as_operator,
                         softplus)


def constraint_greater_than(minval, /):
    """util/gp_util.py:187-201: s -> minval + softplus(s) (torch-style threshold 20)."""

    def constrain(s):
        return minval + softplus(s)

    constrain.minval = minval  # lets the native Gram operator apply the constraint itself
    return constrain


def kernel_scaled_rbf(*, shape_in, shape_out):
    """(parametrize, params_like) with k(x, y) = softplus(raw_s) exp(-|x/l - y/l|^2 / 2), l = softplus(raw_l).

    Same parametrisation as GPyTorch's ScaleKernel(RBFKernel) (util/gp_util.py:151-184).  The returned
    scalar kernel is plain torch (used for small dense checks); the hot path uses ``gram_operator``.
    """
    constrain = constraint_greater_than(0.0)

    def parametrize(*, raw_lengthscale, raw_outputscale):
        def k(x, y):
            _assert_shapes(x, y, shape_in)
            lengthscale = constrain(raw_lengthscale)
            outputscale = constrain(raw_outputscale)
            xs, ys = x / lengthscale, y / lengthscale
            log_k = (xs * xs).sum() + (ys * ys).sum() - 2 * (xs * ys).sum()
            log_k = torch.clamp_min(log_k, 0.0)  # util/gp_util.py:173
            return outputscale * torch.exp(-log_k / 2)

        k.native = ("rbf", raw_lengthscale, raw_outputscale)
        return k

    params_like = {"raw_lengthscale": torch.empty(shape_in), "raw_outputscale": torch.empty(shape_out)}
    return parametrize, params_like


def _scaled_kernel(shape_in, shape_out, radial, kind):
    constrain = constraint_greater_than(0.0)

    def parametrize(*, raw_lengthscale, raw_outputscale):
        def k(x, y):
            _assert_shapes(x, y, shape_in)
            lengthscale = constrain(raw_lengthscale)
            outputscale = constrain(raw_outputscale)
            xs, ys = x / lengthscale, y / lengthscale
            scaled = torch.clamp_min((xs * xs).sum() + (ys * ys).sum() - 2 * (xs * ys).sum(), 0.0)
            return outputscale * radial(scaled)

        k.native = (kind, raw_lengthscale, raw_outputscale)
        return k

    params_like = {"raw_lengthscale": torch.empty(shape_in), "raw_outputscale": torch.empty(shape_out)}
    return parametrize, params_like


def kernel_scaled_matern_32(*, shape_in, shape_out):
    """util/gp_util.py:69-107: (1 + r) exp(-r), r = sqrt(3 |x/l - y/l|^2 + eps).  Hot path: gram_operator(kernel="matern32")."""

    def radial(s):
        r = torch.sqrt(3.0 * s + torch.finfo(s.dtype).eps)
        return (1 + r) * torch.exp(-r)

    return _scaled_kernel(shape_in, shape_out, radial, "matern32")


def kernel_scaled_matern_52(*, shape_in, shape_out):
    """(1 + r + r^2 / 3) exp(-r), r = sqrt(5 |x/l - y/l|^2 + eps): the nu = 5/2 member, with the eps under the root as for
    nu = 1/2 and 3/2 (the reference stops at 3/2).  Hot path: gram_operator(kernel="matern52")."""

    def radial(s):
        r = torch.sqrt(5.0 * s + torch.finfo(s.dtype).eps)
        return (1 + r + r * r / 3) * torch.exp(-r)

    return _scaled_kernel(shape_in, shape_out, radial, "matern52")


def kernel_scaled_matern_12(*, shape_in, shape_out):
    """util/gp_util.py:110-148: exp(-r), r = sqrt(|x/l - y/l|^2 + eps).  Hot path: gram_operator(kernel="matern12")."""

    def radial(s):
        return torch.exp(-torch.sqrt(s + torch.finfo(s.dtype).eps))

    return _scaled_kernel(shape_in, shape_out, radial, "matern12")


def _assert_shapes(x, y, shape_in):
    if tuple(x.shape) != tuple(y.shape):
        error = "The arguments have different shapes: "
        error += f"{tuple(x.shape)} != {tuple(y.shape)})"
        raise ValueError(error)
    if tuple(x.shape) != tuple(shape_in):
        error = f"The shape {tuple(x.shape)} of the first argument "
        error += f"does not match 'shape_in'={shape_in}"
        raise ValueError(error)


def gram_matrix(fun, /):
    """util/gp_util.py:546-549: kernel function -> dense Gram matrix function (small inputs only)."""

    def gram(xs, ys):
        return torch.stack([torch.stack([fun(x, y) for y in ys]) for x in xs])

    return gram


def gram_operator(inputs, *, noise_minval=0.0, precision="f16x3", kernel="rbf"):
    """Matrix-free (K(X, X) + noise I) operator: the native replacement for
    gram_matvec / gram_matvec_partitioned / gram_matvec_sequential applied to the lazy RBF kernel
    with the noise on its diagonal (util/gp_util.py:225-226, 434-543).  No partition count is
    needed: tiles of K live only in registers.

    Use as  ``A = gram_operator(X).bind(raw_lengthscale, raw_outputscale, raw_noise)``.
    """
    return RbfGramOp(inputs, noise_minval=noise_minval, precision=precision, kernel=kernel)


def gram_funm(matfun, krylov_depth, *, precision="f16x3", kernel="rbf", reortho="full", noise_minval=0.0):
    """``apply(inputs, V, raw_lengthscale=, raw_outputscale=, raw_noise=) -> f(K(X, X) + noise I) V`` for V (n,) or (p, n), by
    ``lanczos.funm_spd`` on the native Gram operator (the constrain / ``gram_operator`` plumbing of the likelihoods).  With z ~ N(0, I),
    ``matfun=torch.sqrt`` gives prior draws from N(0, K + sigma^2 I) and ``matfun=torch.rsqrt`` whitens residuals.  Differentiable w.r.t.
    the raw parameters, V and the inputs.  No counterpart in the reference."""

    def apply(inputs, V, *, raw_lengthscale, raw_outputscale, raw_noise):
        op = gram_operator(inputs, noise_minval=noise_minval, precision=precision, kernel=kernel)
        funm = lanczos.funm_spd(matfun, krylov_depth, op.bind(raw_lengthscale, raw_outputscale, raw_noise), reortho=reortho)
        return funm(V)

    return apply


def krylov_logdet_slq(krylov_depth, /, *, sample, num_batches: int, checkpoint: bool = False):
    """util/gp_util.py:552-576: logdet(A, key) -> (value, info) by stochastic Lanczos quadrature.

    ``checkpoint`` is accepted for signature parity; rematerialisation is a JAX memory device, the
    HIP path stores the (p, k, n) basis once and never materialises kernel tiles.
    """

    def logdet(A, /, key):
        integrand = lanczos.integrand_spd(torch.log, krylov_depth, A)
        estimate = hutchinson.hutchinson(integrand, sample)
        if num_batches == 1:
            value = estimate(key)
            return value, {"std": 0.0, "std_rel": 0.0}
        keys = hutchinson.split(key, num_batches)
        values = torch.stack([estimate(k) for k in keys])
        mean = values.mean(dim=0)
        std = values.std(dim=0, unbiased=False)
        return mean, {"std_abs": std, "std_rel": std / mean.abs()}

    return logdet


def krylov_logdet_slq_p(krylov_depth, /, *, sample, num_batches: int):
    """logdet(A, key, P=...) -> (value, info): the SLQ log-determinant on the preconditioned operator.

    For the SPD preconditioner P that likelihood_pdf_p builds (a ``low_rank.BoundPreconditioner``) and S = P^-1/2 held constant,
    log det A = log det P + tr log(S A S): the value is ``P.logdet()`` plus ``krylov_logdet_slq`` on ``PreconditionedOp``, whose
    spectrum clusters at 1 -- a small ``krylov_depth`` converges, and far deeper ones break down as the reference's recurrence does.
    ``A`` is a bound native operator.  Differentiable with respect to everything ``krylov_logdet_slq`` is (the inputs X of a
    kernel-Gram operator included), with the gradient of log det A itself; no gradient flows through P.  No counterpart in the
    reference."""
    slq = krylov_logdet_slq(krylov_depth, sample=sample, num_batches=num_batches)

    def logdet(A, /, key, *, P):
        if not (isinstance(A, BoundOp) and isinstance(A.op, NativeOp)):
            raise TypeError("krylov_logdet_slq_p: A must be a bound native operator (op.bind(*params))")
        if not isinstance(P, low_rank.BoundPreconditioner):
            raise TypeError("krylov_logdet_slq_p: P must be the bound preconditioner likelihood_pdf_p passes (pre.bind(noise))")
        B = PreconditionedOp(A.op, P.pre, P.s)
        value, info = slq(B.bind(*A.params), key)
        return value + B.logdet().to(value.dtype), info

    return logdet


def krylov_logdet_slq_vjp_reuse(krylov_depth, /, *, sample, num_batches: int, checkpoint: bool = False):
    """util/gp_util.py:579-621: same value, cheap inexact gradient (re-used Lanczos basis)."""

    def logdet(A, /, key):
        integrand = lanczos.integrand_spd_custom_vjp_reuse(torch.log, krylov_depth, A)
        estimate = hutchinson.hutchinson(integrand, sample)
        keys = hutchinson.split(key, num_batches)
        values = torch.stack([estimate(k) for k in keys])
        return values.mean(dim=0), {"std": values.std(dim=0, unbiased=False)}

    return logdet


# ------------------------------------------------------------------------------------------------
# "next" tier: the log-marginal likelihood around the SLQ log-determinant and the PCG solve
# ------------------------------------------------------------------------------------------------
def target_logml(model, likelihood, /):
    """util/gp_util.py:15-32."""

    def mll(inputs, targets, *p_logpdf, params_mean: dict, params_kernel: dict, params_likelihood: dict):
        mean, kernel = model(params_mean=params_mean, params_kernel=params_kernel)
        loss = likelihood(inputs, mean=mean, kernel=kernel, params=params_likelihood)
        value, info_pdf = loss(targets, *p_logpdf)
        return value, info_pdf

    return mll


def model_gp(mean_fun, kernel_fun):
    """util/gp_util.py:48-56."""

    def prior(params_mean: dict, params_kernel: dict):
        return mean_fun(**params_mean), kernel_fun(**params_kernel)

    return prior


def mean_constant(*, shape_out):
    """util/gp_util.py:59-66."""

    def parametrize(*, constant_value):
        def mean(_x):
            return constant_value

        mean.batched = lambda xs: constant_value.expand((xs.shape[0], *constant_value.shape))
        return mean

    return parametrize, {"constant_value": torch.empty(shape_out)}


def _mean_array(mean, inputs):
    if hasattr(mean, "batched"):
        return mean.batched(inputs)
    return torch.stack([mean(x) for x in inputs])


class _GramStrategy:
    """What gram_matvec* return here: the matvec strategy is always the native matrix-free operator."""

    def __init__(self, precision="f16x3"):
        self.precision = precision


def gram_matvec(*, precision="f16x3"):
    """util/gp_util.py:525-543."""
    return _GramStrategy(precision)


def gram_matvec_partitioned(num: int = 1, *, checkpoint: bool = False, precision="f16x3"):
    """util/gp_util.py:470-522; ``num`` / ``checkpoint`` are accepted for signature parity (no Gram tile ever reaches HBM)."""
    return _GramStrategy(precision)


def gram_matvec_sequential(*, checkpoint: bool = False, precision="f16x3"):
    """util/gp_util.py:434-467."""
    return _GramStrategy(precision)


def _native_cov(matvec, inputs, kernel, constrain, raw_noise):
    if not hasattr(kernel, "native"):
        raise TypeError("the kernel must come from kernel_scaled_rbf / kernel_scaled_matern_52 / kernel_scaled_matern_32 / kernel_scaled_matern_12 "
                        "(the native Gram operator evaluates it on the device)")
    if not hasattr(constrain, "minval"):
        raise TypeError("constrain must come from constraint_greater_than")
    kind, raw_lengthscale, raw_outputscale = kernel.native
    precision = matvec.precision if isinstance(matvec, _GramStrategy) else "f16x3"
    op = RbfGramOp(inputs, noise_minval=constrain.minval, precision=precision, kernel=kind)
    return op.bind(raw_lengthscale, raw_outputscale, raw_noise)


def likelihood_pdf(matvec, logpdf, *, constrain):
    """Gaussian likelihood, noise inside the lazy kernel (util/gp_util.py:216-240)."""

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])

        def logpdf_partial(targets, *p_logpdf):
            return logpdf(targets, *p_logpdf, mean=_mean_array(mean, inputs), cov_matvec=cov_matvec)

        return logpdf_partial

    return likelihood, {"raw_noise": torch.empty(())}


def likelihood_pdf_p(matvec, logpdf_p, precondition, *, constrain):
    """Gaussian likelihood with a preconditioner built from the NOISE-FREE kernel (util/gp_util.py:243-276)."""

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])
        noise = constrain(params["raw_noise"])
        pre, info = precondition(low_rank.without_noise(cov_matvec), len(inputs))

        def logpdf_partial(targets, *p_logpdf):
            val, aux = logpdf_p(targets, *p_logpdf, mean=_mean_array(mean, inputs), cov_matvec=cov_matvec,
                                P=pre.bind(noise))
            return val, {"precondition": info, "logpdf": aux}

        return logpdf_partial

    return likelihood, {"raw_noise": torch.empty(())}


def logpdf_scipy_stats():
    """Dense reference (util/gp_util.py:354-364: jax.scipy.stats.multivariate_normal.logpdf of the materialised covariance) -- here
    torch.distributions.MultivariateNormal on the same materialised matrix; used by the reference's gpytorch comparison test and its
    fixed-step training script (optim_logml_adjoints_fixed.py:136) as the exact baseline."""

    def logpdf(y, /, *, mean, cov_matvec):
        n = mean.shape[0]
        cov_matrix = cov_matvec(torch.eye(n, dtype=mean.dtype, device=mean.device)).t()
        cov_matrix = 0.5 * (cov_matrix + cov_matrix.t())  # (the distribution insists on exact symmetry)
        return torch.distributions.MultivariateNormal(mean, covariance_matrix=cov_matrix).log_prob(y), {}

    return logpdf


def logpdf_cholesky():
    """Dense baseline (util/gp_util.py:367-393): materialise the covariance through the operator, then Cholesky."""

    def logpdf(y, /, *, mean, cov_matvec):
        n = mean.shape[0]
        cov_matrix = cov_matvec(torch.eye(n, dtype=mean.dtype, device=mean.device)).t()
        cholesky = torch.linalg.cholesky(cov_matrix)
        logdet = torch.log(torch.diagonal(cholesky)).sum()
        tmp = torch.linalg.solve_triangular(cholesky, (y - mean)[:, None], upper=False)[:, 0]
        mahalanobis = tmp @ tmp
        return -logdet - 0.5 * mahalanobis - n / 2 * math.log(2 * math.pi), {}

    return logpdf


def logpdf_krylov(solve, logdet):
    """util/gp_util.py:396-411."""

    def logpdf(y, *params_logdet, mean, cov_matvec):
        logdet_, info_logdet = logdet(cov_matvec, *params_logdet)
        logdet_ = logdet_ / 2
        tmp, info_solve = solve(cov_matvec, y - mean)
        mahalanobis = (y - mean) @ tmp
        info = {"logdet": info_logdet, "solve": info_solve}
        (n,) = mean.shape
        return -logdet_ - 0.5 * mahalanobis - n / 2 * math.log(2 * math.pi), info

    return logpdf


def logpdf_krylov_p(solve_p, logdet):
    """util/gp_util.py:414-431."""

    def logpdf(y, *params_logdet, mean, cov_matvec, P):
        logdet_, info_logdet = logdet(cov_matvec, *params_logdet)
        logdet_ = logdet_ / 2
        tmp, info_solve = solve_p(cov_matvec, y - mean, P=P)
        mahalanobis = (y - mean) @ tmp
        info = {"logdet": info_logdet, "solve": info_solve}
        (n,) = mean.shape
        return -logdet_ - 0.5 * mahalanobis - n / 2 * math.log(2 * math.pi), info

    return logpdf


def logpdf_krylov_pslq(solve_p, logdet_p):
    """``logpdf_krylov_p`` with the preconditioner forwarded to the log-determinant as well (``krylov_logdet_slq_p``)."""

    def logpdf(y, *params_logdet, mean, cov_matvec, P):
        logdet_, info_logdet = logdet_p(cov_matvec, *params_logdet, P=P)
        logdet_ = logdet_ / 2
        tmp, info_solve = solve_p(cov_matvec, y - mean, P=P)
        mahalanobis = (y - mean) @ tmp
        info = {"logdet": info_logdet, "solve": info_solve}
        (n,) = mean.shape
        return -logdet_ - 0.5 * mahalanobis - n / 2 * math.log(2 * math.pi), info

    return logpdf


# ------------------------------------------------------------------------------------------------
# modified batched CG (mBCG): log-determinant and log-likelihood from ONE preconditioned solve  
# ------------------------------------------------------------------------------------------------
def _mbcg_config(solve_mbcg):
    cfg = getattr(solve_mbcg, "cfg", None)
    if not (isinstance(cfg, dict) and cfg.get("mbcg", False)):
        raise TypeError("solve_mbcg must come from cg.mbcg_fixed_step / cg.mbcg_adaptive (the solver that keeps its coefficients)")
    return cfg


def _mbcg_probes(op, cparams, key, P, num_probes):
    """(num_probes, n) probes with covariance M: an explicit tensor as it is (the parity interface of ``hutchinson``), else
    ``P.sample`` (M = s I + L L^T), else plain +-1 (M = I); ``key`` an int seed or (seed, first_probe)."""
    if torch.is_tensor(key):
        if key.dim() != 2 or key.shape[0] != num_probes:
            raise ValueError(f"explicit probes {tuple(key.shape)} must be ({num_probes}, n)")
        return key.detach()
    seed, first = key if isinstance(key, tuple) else (key, 0)
    if P is not None:
        return P.sample(seed, num_probes, first_probe=first)
    if isinstance(op, CallbackOp):
        raise TypeError("a callable operator has no size: pass explicit probes (num_probes, n) as the key")
    ref = next(q for q in cparams if torch.is_tensor(q))
    like = torch.empty(op.size(*cparams), dtype=ref.dtype, device=ref.device)
    return hutchinson.sampler_rademacher(like, num=num_probes)((seed, first))


def _mbcg_quadrature(tdiag, toff, rz0, kmax=None):
    """rz0_b e1^T log(T_b) e1 per right-hand side, in fp64, for the padded tridiagonals of ``mfx_mbcg_solve`` (the identity block
    beyond a column's depth has log 1 = 0 and no weight on e1).  ``kmax``: only the leading kmax x kmax block can be live."""
    p, k = tdiag.shape
    if kmax is not None and kmax < k:
        k = max(int(kmax), 1)
        tdiag, toff = tdiag[:, :k], toff[:, :k]
    dt, dev = tdiag.dtype, tdiag.device
    # beyond depth 120 the eigensolver accumulates its rotations in the fp64 output itself (include/mfx.h): fp32 problems are cast
    et = torch.float64 if k > 120 else dt
    diag_e, off_e = tdiag.to(et).contiguous(), toff.to(et).contiguous()
    evals = torch.empty((p, k), dtype=et, device=dev)
    evecs = torch.empty((p, k, k), dtype=et, device=dev)
    _lib.check(_lib.get().mfx_tridiag_eigh(_lib.ptr(diag_e), _lib.ptr(off_e) if k > 1 else None, k, p, k, _lib.dtype_code(et),
                                           _lib.ptr(evals), _lib.ptr(evecs), _lib.stream_ptr(dev)))
    weights = evecs[:, 0, :].double() ** 2
    return rz0.double() * (weights * torch.log(evals.double())).sum(-1)


def _mbcg_kmax(cfg, steps):
    # the adaptive loop has synchronised with the host every iteration anyway: trim the eigen-problem to the steps taken
    return int(steps.max()) if cfg["adaptive"] else None


def krylov_logdet_mbcg(solve_mbcg, /, *, num_probes: int):
    """logdet(A, key, P=None) -> (value, info): the log-determinant estimate of modified batched CG (the estimator of GPyTorch
    that the reference's optim_logml_gpytorch_adaptive.py trains with).  One ``solve_mbcg`` (cg.mbcg_fixed_step / cg.mbcg_adaptive)
    on ``num_probes`` probes z_b with covariance M (the preconditioner ``P = pre.bind(s)``, M = s I + L L^T; M = I for None):

        value = logdet M + (1 / p) sum_b rz0_b e1^T log(T_b) e1,

    T_b the Lanczos tridiagonal of M^-1/2 A M^-1/2 started at M^-1/2 z_b that the CG coefficients form, rz0_b = z_b^T M^-1 z_b.
    ``key``: int seed, (seed, first_probe), or the probes themselves.  The value carries no gradient: ``logpdf_mbcg`` owns it."""
    cfg = _mbcg_config(solve_mbcg)
    num_probes = int(num_probes)
    if num_probes < 1:
        raise ValueError(f"num_probes must be >= 1, got {num_probes}")

    def logdet(A, /, key, P=None):
        op, bound = as_operator(A)
        cg._check_mbcg(op, P, cfg)
        with torch.no_grad():
            cparams = op.constrain(*(tuple(bound) if bound is not None else ()))
            z = _mbcg_probes(op, cparams, key, P, num_probes)
            _x, info = solve_mbcg(A, z, P)
            quad = _mbcg_quadrature(*info["tridiag"], info["rz0"], _mbcg_kmax(cfg, info["num_steps"]))
            value = quad.mean()
            if P is not None:
                value = value + P.logdet()
            std = quad.std(unbiased=False)
        return value.to(z.dtype), {"std_abs": std, "std_rel": std / value.abs(), "solve": info}

    return logdet


class _MbcgLogpdfFn(torch.autograd.Function):
    """value = -1/2 r^T A^-1 r - 1/2 logdet A - n/2 log 2 pi from ONE mfx_mbcg_solve on [r ; z_1 .. z_p]."""

    @staticmethod
    def forward(ctx, op, cfg, P, z, y, mean, *cparams):
        tensors = [q for q in cparams if torch.is_tensor(q)]
        _lib.require_device(y, z, *tensors)
        resid = (y - mean).to(z.dtype)
        n, p = resid.shape[0], z.shape[0]
        B = torch.cat([resid[None], z])
        x, r, steps, tdiag, toff, rz0, depth, w0 = cg._run(op, cfg, P, B, cparams)
        quad = _mbcg_quadrature(tdiag[1:], toff[1:], rz0[1:], _mbcg_kmax(cfg, steps[1:]))
        logdet = quad.mean()
        if P is not None:
            logdet = logdet + P.logdet()
        value = -0.5 * (resid.double() @ x[0].double()) - 0.5 * logdet - n / 2 * math.log(2 * math.pi)
        ctx.op, ctx.p = op, p
        ctx.nontensor = [None if torch.is_tensor(q) else q for q in cparams]
        ctx.save_for_backward(x, w0, *tensors)
        out = (r, steps, depth, logdet.to(z.dtype))
        ctx.mark_non_differentiable(*out)
        return (value.to(z.dtype), *out)

    @staticmethod
    def backward(ctx, g, *_unused):
        x, w0, *tensors = ctx.saved_tensors
        it = iter(tensors)
        cparams = tuple(next(it) if q is None else q for q in ctx.nontensor)
        op, p = ctx.op, ctx.p
        if isinstance(op, CallbackOp):
            raise NotImplementedError("logpdf_mbcg differentiates native operators only (the gradient is ONE mfx_op_vjp_params sweep, "
                                      "which a Python callable does not have)")
        n = x.shape[1]
        alpha = x[:1]
        # d/dtheta [1/2 alpha^T A alpha - 1/(2p) sum_b x_b^T A w_b]:  tr(A^-1 dA) ~ mean_b z_b^T M^-1 dA A^-1 z_b for E[z z^T] = M
        L = torch.cat([0.5 * g * alpha, (-0.5 / p) * g * x[1:]]).contiguous()
        R = torch.cat([alpha, w0[1:]]).contiguous()
        desc = op.descriptor(cparams, x.dtype, n)
        gstruct, grads = op.new_grads(*cparams)
        ws = _lib.workspace(desc, n, 1, p + 1, x.device)
        _lib.check(_lib.get().mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), n, _lib.ptr(R), n, p + 1, C.byref(gstruct),
                                                _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
        galpha = g * alpha[0]  # d value / d y = -alpha, d value / d mean = +alpha  (r = y - mean)
        return (None, None, None, None, -galpha, galpha, *grads)


def logpdf_mbcg(solve_mbcg, /, *, num_probes: int):
    """logpdf(y, key, *, mean, cov_matvec, P=None) -> (value, info): the Gaussian log-density by modified batched CG, usable under
    both ``likelihood_pdf`` and ``likelihood_pdf_p`` (where ``logpdf_krylov[_p]`` runs an SLQ pass beside a separate solve).

    ONE ``mfx_mbcg_solve`` on the num_probes + 1 right-hand sides [y - mean ; z_1 .. z_p], z_b probes with the preconditioner's
    covariance M (``P.sample``; plain +-1 without P):
        value = -1/2 r^T alpha - 1/2 logdet - n/2 log 2 pi,   r = y - mean,  alpha = A^-1 r,  logdet as ``krylov_logdet_mbcg``.
    Backward, with x_b = A^-1 z_b and w_b = M^-1 z_b from the same solve: ONE parameter sweep (``mfx_op_vjp_params``, the input
    gradient included when X.requires_grad) of  1/2 alpha^T dA alpha - 1/(2p) sum_b x_b^T dA w_b;  -alpha to y, +alpha to the mean.

    The gradient of the log-determinant term is the TRACE ESTIMATOR tr(A^-1 dA) ~ mean_b x_b^T dA w_b (unbiased for any fixed M when
    the solves have converged) -- it is NOT the derivative of the forward quadrature, so value and gradient are two estimates from
    the same probes, not a function and its derivative (a finite-difference check of the value does not reproduce it).  Nothing flows
    through the preconditioner (``low_rank._NoGrad`` convention).  Native operators only: a callable operator raises
    NotImplementedError in backward.  ``key``: int seed, (seed, first_probe) or explicit probes (num_probes, n)."""
    cfg = _mbcg_config(solve_mbcg)
    num_probes = int(num_probes)
    if num_probes < 1:
        raise ValueError(f"num_probes must be >= 1, got {num_probes}")

    def logpdf(y, key, *, mean, cov_matvec, P=None):
        op, bound = as_operator(cov_matvec)
        cg._check_mbcg(op, P, cfg)
        cparams = op.constrain(*(tuple(bound) if bound is not None else ()))
        with torch.no_grad():
            z = _mbcg_probes(op, cparams, key, P, num_probes)
        value, r, steps, depth, logdet = _MbcgLogpdfFn.apply(op, cfg, P, z, y, mean, *cparams)
        solve = {"residual_abs": r[0], "num_steps": steps[0]}
        return value, {"logdet": {"value": logdet, "depth": depth[1:], "num_steps": steps[1:], "residual_abs": r[1:]},
                       "solve": solve}

    return logpdf


def target_posterior(model, likelihood, /):
    """util/gp_util.py:35-45: -> posterior(inputs, targets, params_mean, params_kernel, params_likelihood) -> (predict, {})
    with predict(xs) -> (posterior mean at xs, info)."""

    def posterior(inputs, targets, params_mean: dict, params_kernel: dict, params_likelihood: dict):
        mean, kernel = model(params_mean, params_kernel)
        condition = likelihood(inputs, mean, kernel, params=params_likelihood)
        return (lambda xs: condition(xs, targets=targets)), {}

    return posterior


def likelihood_condition(matvec, solve, *, constrain):
    """util/gp_util.py:279-310: weights = solve(K + noise I, y - m);  prediction = m(xs) + K(xs, X) weights."""

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])

        def condition_partial(xs, targets):
            weights, info = solve(cov_matvec, targets - _mean_array(mean, inputs))
            return _mean_array(mean, xs) + cov_matvec.op.cross_apply(xs, weights, *cov_matvec.params), {"solve": info}

        return condition_partial

    return likelihood, {"raw_noise": torch.empty(())}


def likelihood_condition_p(matvec, solve_p, *, precondition, constrain):
    """util/gp_util.py:313-351: the same with a preconditioned solve."""

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])
        noise = constrain(params["raw_noise"])
        pre, _info = precondition(low_rank.without_noise(cov_matvec), len(inputs))

        def condition_partial(xs, targets):
            weights, info = solve_p(cov_matvec, targets - _mean_array(mean, inputs), P=pre.bind(noise))
            return _mean_array(mean, xs) + cov_matvec.op.cross_apply(xs, weights, *cov_matvec.params), {"solve": info}

        return condition_partial

    return likelihood, {"raw_noise": torch.empty(())}


def _refuse_sharded_paths(A):
    op = A.op if isinstance(A, BoundOp) else A
    if isinstance(op, RowShardedOp):
        raise NotImplementedError("pathwise posterior samples are not available on row-sharded operators (the random features and "
                                  "K(xs, X) need the whole operator); use the operator itself, or shard the samples")


class PathwisePosterior:
    """S posterior sample paths of a GP by Matheron's rule, as functions: ``paths(xs)`` -> (S, len(xs)), and a second call at other
    points evaluates the SAME S functions there.

        f_s(x*) = m(x*) + phi(x*) . w_s + K(x*, X) v_s,    v_s = (K + noise I)^-1 (y - m(X) - phi(X) . w_s - eps_s)

    The representer weights v (S, n) come from ONE batched solve at construction (``info["solve"]``) and are constants afterwards.
    An evaluation is one RandomFeatures.evaluate, one RbfGramOp.cross_apply with the S weight vectors, and the mean; it is
    differentiable with respect to xs (nothing else: the hyper-parameters must not require grad)."""

    def __init__(self, cov_matvec, solve, mean, features, inputs, targets, *, key=None, eps=None):
        _refuse_sharded_paths(cov_matvec)
        op = cov_matvec.op if isinstance(cov_matvec, BoundOp) else None
        if not isinstance(op, RbfGramOp):
            raise TypeError("PathwisePosterior needs a bound RbfGramOp (gram_operator(X).bind(...)): the features follow its kernel")
        if features.kernel != op.kernel or features.dim != op.d:
            raise ValueError(f"PathwisePosterior: the features are for kernel {features.kernel!r} in {features.dim} dimensions, the "
                             f"operator has kernel {op.kernel!r} in {op.d}")
        S, n = features.num_samples, op.n
        ls, s, nz = op.constrain(*cov_matvec.params)[:3]
        self.cov_matvec, self.mean, self.features = cov_matvec, mean, features
        self.lengthscale, self.outputscale = ls, s
        with torch.no_grad():
            prior = features.evaluate(op.X.detach(), ls, s)  # (S, n); refuses hyper-parameters that require grad
            if eps is None:
                if key is None or torch.is_tensor(key):
                    raise ValueError("PathwisePosterior: the noise draws eps need an integer key (or (seed, offset)); or pass eps= "
                                     f"({S}, {n}) explicitly")
                eps = hutchinson.sampler_normal(op.X[:, 0], num=S)(key) * torch.sqrt(nz)
            if tuple(eps.shape) != (S, n):
                raise ValueError(f"PathwisePosterior: eps {tuple(eps.shape)} must be ({S}, {n})")
            residual = (targets - _mean_array(mean, inputs)).reshape(1, n).to(prior.dtype)
            weights, info = solve(cov_matvec, residual - prior - eps.to(prior.dtype))
        self.weights, self.info = weights.detach(), {"solve": info}

    def __call__(self, xs):
        op = self.cov_matvec.op
        xs = xs.to(op.X.dtype)
        prior = self.features.evaluate(xs, self.lengthscale, self.outputscale)
        update = op.cross_apply(xs, self.weights, *self.cov_matvec.params)
        return _mean_array(self.mean, xs).reshape(1, -1) + prior + update


def _pathwise_likelihood(matvec, solve_with, constrain, num_samples, num_features, key, omega, phase, weights, eps):
    _refuse_sharded_paths(matvec)
    if int(num_samples) < 1 or int(num_features) < 1:
        raise ValueError(f"num_samples and num_features must be >= 1, got {num_samples} and {num_features}")
    if torch.is_tensor(key):
        raise ValueError("the key must be an integer seed (or (seed, offset)): explicit draws go in omega=, phase=, weights= and eps=")
    explicit = {"omega": omega, "phase": phase, "weights": weights, "eps": eps}
    if key is None and any(t is None for t in explicit.values()):
        raise ValueError(f"key=None needs every draw given explicitly; missing: {', '.join(k for k, t in explicit.items() if t is None)}")
    key_features, key_eps = (None, None) if key is None else hutchinson.split(key, 2)

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])
        features = RandomFeatures(key_features, kernel=cov_matvec.op.kernel, dim=cov_matvec.op.d, num_features=num_features,
                                  num_samples=num_samples, like=cov_matvec.op.X, omega=omega, phase=phase, weights=weights)
        solve = solve_with(cov_matvec, constrain(params["raw_noise"]), len(inputs))

        def condition_partial(xs, targets):
            paths = PathwisePosterior(cov_matvec, solve, mean, features, inputs, targets, key=key_eps, eps=eps)
            return paths, paths.info

        return condition_partial

    return likelihood, {"raw_noise": torch.empty(())}


def likelihood_condition_pathwise(matvec, solve, *, constrain, num_samples, num_features, key, omega=None, phase=None, weights=None,
                                  eps=None):
    """likelihood_condition that draws posterior FUNCTIONS: condition(xs, targets) -> (paths, info), paths a PathwisePosterior --
    ``paths(points)`` -> (num_samples, len(points)), callable again at other points for the same functions, differentiable with
    respect to the points.  ``xs`` is accepted for target_posterior's signature and not used: nothing is evaluated until
    ``paths`` is called.  One batched solve with num_samples right-hand sides per condition() call (info["solve"]).

    The num_features random features (operators.RandomFeatures) and the noise draws eps ~ N(0, noise I) come from ``key`` (split in
    two); explicit ``omega=, phase=, weights=`` (m, d), (m,), (S, m) and ``eps=`` (S, n) -- the draws themselves, variance noise --
    are taken as given.  Refused: a RowShardedOp (before any collective), hyper-parameters that require grad (ValueError from
    RandomFeatures.evaluate).  Known limit: a finite num_features under-represents the prior variance far from the data."""
    return _pathwise_likelihood(matvec, lambda _cov, _noise, _n: solve, constrain, num_samples, num_features, key, omega, phase, weights,
                                eps)


def likelihood_condition_pathwise_p(matvec, solve_p, *, precondition, constrain, num_samples, num_features, key, omega=None, phase=None,
                                    weights=None, eps=None):
    """likelihood_condition_pathwise with a preconditioned solve, as likelihood_condition_p."""

    def solve_with(cov_matvec, noise, n):
        pre, _info = precondition(low_rank.without_noise(cov_matvec), n)
        return lambda A, B: solve_p(A, B, P=pre.bind(noise))

    return _pathwise_likelihood(matvec, solve_with, constrain, num_samples, num_features, key, omega, phase, weights, eps)


def _predictive_variance(cov_matvec, solve, xs, noise, observation_noise, chunk):
    """the clamped predictive variance of likelihood_condition_var[_p] and its info"""
    latent, info = cov_matvec.op.posterior_variance(xs, solve, *cov_matvec.params, chunk=chunk, return_info=True)
    clamped = latent < 0
    var = latent.clamp_min(0.0)
    if observation_noise:
        var = var + noise.to(var.dtype)
    return var, {"variance_solve": info["solve"], "num_clamped": clamped.sum()}


def _check_chunk(chunk):
    if int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    return int(chunk)


def likelihood_condition_var(matvec, solve, *, constrain, observation_noise=False, chunk=64):
    """likelihood_condition with the predictive variance: condition(xs, targets) -> ((mean, variance), info).

    mean is likelihood_condition's.  variance = max(0, s kappa(0) - diag(K(xs, X) A^-1 K(X, xs))) (RbfGramOp.posterior_variance,
    ``chunk`` test points per batched solve), plus the noise when observation_noise (the variance of a noisy observation; the noise
    then gets its gradient).  info = {"solve": the mean's solve info, "variance_solve": the solver's info per test point,
    "num_clamped": how many variances were negative by rounding and clamped to 0}."""
    chunk = _check_chunk(chunk)

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])
        noise = constrain(params["raw_noise"])

        def condition_partial(xs, targets):
            weights, info = solve(cov_matvec, targets - _mean_array(mean, inputs))
            mu = _mean_array(mean, xs) + cov_matvec.op.cross_apply(xs, weights, *cov_matvec.params)
            var, vinfo = _predictive_variance(cov_matvec, solve, xs, noise, observation_noise, chunk)
            return (mu, var), {"solve": info, **vinfo}

        return condition_partial

    return likelihood, {"raw_noise": torch.empty(())}


def likelihood_condition_var_p(matvec, solve_p, *, precondition, constrain, observation_noise=False, chunk=64):
    """likelihood_condition_p with the predictive variance, as likelihood_condition_var (the variance solves take the same
    preconditioner as the mean's)."""
    chunk = _check_chunk(chunk)

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])
        noise = constrain(params["raw_noise"])
        pre, _info = precondition(low_rank.without_noise(cov_matvec), len(inputs))

        def condition_partial(xs, targets):
            weights, info = solve_p(cov_matvec, targets - _mean_array(mean, inputs), P=pre.bind(noise))
            mu = _mean_array(mean, xs) + cov_matvec.op.cross_apply(xs, weights, *cov_matvec.params)
            var, vinfo = _predictive_variance(cov_matvec, lambda A, B: solve_p(A, B, P=pre.bind(noise)), xs, noise,
                                              observation_noise, chunk)
            return (mu, var), {"solve": info, **vinfo}

        return condition_partial

    return likelihood, {"raw_noise": torch.empty(())}


def _predictive_covariance(cov_matvec, solve, xs, noise, observation_noise, chunk):
    """the joint predictive covariance of likelihood_condition_cov[_p] and its info"""
    cov, info = cov_matvec.op.posterior_covariance(xs, solve, *cov_matvec.params, chunk=chunk, return_info=True)
    if observation_noise:
        cov = cov + torch.diag_embed(noise.to(cov.dtype).reshape(1).expand(cov.shape[0]))
    return cov, {"covariance_solve": info["solve"]}


def likelihood_condition_cov(matvec, solve, *, constrain, observation_noise=False, chunk=64):
    """likelihood_condition with the joint predictive covariance: condition(xs, targets) -> ((mean, covariance), info).

    mean is likelihood_condition's.  covariance = K(xs, xs) - K(xs, X) A^-1 K(X, xs) (RbfGramOp.posterior_covariance, ``chunk``
    test points per batched solve; (m, m), bitwise symmetric, neither clamped nor jittered), plus the noise on its diagonal when
    observation_noise (the covariance of noisy observations; the noise then gets its gradient through that term too).
    info = {"solve": the mean's solve info, "covariance_solve": the solver's info per test point}.  Draws: posterior_samples."""
    chunk = _check_chunk(chunk)

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])
        noise = constrain(params["raw_noise"])

        def condition_partial(xs, targets):
            weights, info = solve(cov_matvec, targets - _mean_array(mean, inputs))
            mu = _mean_array(mean, xs) + cov_matvec.op.cross_apply(xs, weights, *cov_matvec.params)
            cov, cinfo = _predictive_covariance(cov_matvec, solve, xs, noise, observation_noise, chunk)
            return (mu, cov), {"solve": info, **cinfo}

        return condition_partial

    return likelihood, {"raw_noise": torch.empty(())}


def likelihood_condition_cov_p(matvec, solve_p, *, precondition, constrain, observation_noise=False, chunk=64):
    """likelihood_condition_p with the joint predictive covariance, as likelihood_condition_cov (the covariance solves take the
    same preconditioner as the mean's)."""
    chunk = _check_chunk(chunk)

    def likelihood(inputs, mean, kernel, params: dict):
        cov_matvec = _native_cov(matvec, inputs, kernel, constrain, params["raw_noise"])
        noise = constrain(params["raw_noise"])
        pre, _info = precondition(low_rank.without_noise(cov_matvec), len(inputs))

        def condition_partial(xs, targets):
            weights, info = solve_p(cov_matvec, targets - _mean_array(mean, inputs), P=pre.bind(noise))
            mu = _mean_array(mean, xs) + cov_matvec.op.cross_apply(xs, weights, *cov_matvec.params)
            cov, cinfo = _predictive_covariance(cov_matvec, lambda A, B: solve_p(A, B, P=pre.bind(noise)), xs, noise,
                                                observation_noise, chunk)
            return (mu, cov), {"solve": info, **cinfo}

        return condition_partial

    return likelihood, {"raw_noise": torch.empty(())}


def posterior_samples(key, mean, cov, *, num, jitter=0.0):
    """``num`` draws mean + L eps from N(mean, cov) -> (num, m), with L = cholesky(cov + jitter I) factored in fp64 on the device
    of ``cov`` and cast back to its dtype, and eps (num, m) standard normal drawn from ``key`` as hutchinson.sampler_normal draws
    it (the same key gives the same draws; an explicit (num, m) tensor is taken as eps itself).  Plain torch, so differentiable
    with respect to mean and cov.  A predictive covariance is positive semi-definite only up to rounding and the solver's
    tolerance: a factorisation that fails raises ValueError -- pass a (larger) ``jitter``."""
    num = int(num)
    if num < 1:
        raise ValueError(f"posterior_samples: num must be >= 1, got {num}")
    if mean.dim() != 1 or cov.dim() != 2 or cov.shape != (mean.shape[0], mean.shape[0]):
        raise ValueError(f"posterior_samples: mean {tuple(mean.shape)} and cov {tuple(cov.shape)} must be (m,) and (m, m)")
    m = mean.shape[0]
    shifted = cov.double() + float(jitter) * torch.eye(m, dtype=torch.float64, device=cov.device)
    L, failed = torch.linalg.cholesky_ex(shifted)
    if int(failed) != 0:
        raise ValueError(f"posterior_samples: cov + jitter I is not positive definite (jitter = {jitter}; the factorisation stopped "
                         f"at leading minor {int(failed)}); pass a larger jitter")
    eps = hutchinson.sampler_normal(mean, num=num)(key)
    if tuple(eps.shape) != (num, m):
        raise ValueError(f"posterior_samples: explicit draws {tuple(eps.shape)} must be ({num}, {m})")
    return mean + eps.to(cov.dtype) @ L.to(cov.dtype).T
