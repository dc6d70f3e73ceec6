"""Lanczos tridiagonalisation with adjoints and the SLQ integrand -- MI355X build.

Same functional surface as the reference's ``matfree_extensions/lanczos.py``:

    tridiag(matvec, krylov_depth, /, *, reortho, custom_vjp=True)
        -> estimate(vec, *params) -> ((basis (k, n), (diag (k,), offdiag (k-1,))), (q (n,), beta ()))
    integrand_spd(matfun, krylov_depth, matvec, /, *, reortho="full", use_adjoints_for_tridiag=True)
        -> quadform(v0, *params) -> scalar
    integrand_spd_custom_vjp_reuse(matfun, order, matvec, /, *, reortho="full")

and, beyond the reference, the vector-valued form on the same path:

    funm_spd(matfun, krylov_depth, matvec, /, *, reortho="full", custom_vjp=True)
        -> apply(v, *params) -> f(A) v  (``mfx_funm_coeffs`` / ``mfx_basis_combine`` and their VJPs)

``reortho="full"`` runs through the Arnoldi kernels exactly as the reference does (lanczos.py:152-169);
``reortho="none"`` is the three-term recurrence with its own adjoint (lanczos.py:172-335).  The k x k
eigen-problem and its VJP (lanczos.py:48-59) run on the device too (``mfx_tridiag_eigh`` /
``mfx_slq_quadform_bwd``).  Vectors may be batched (p, n): every output gains a leading probe axis.
"""

from __future__ import annotations

import warnings

import torch

from . import _lib, arnoldi
from .operators import (CallbackOp, DriverCall, RowShardedOp, as_operator, differentiable_inputs, rebuild_params, reduce_grads_,
                        stash_params, with_inputs)


def _vec_norm(V, matvec):
    """Euclidean norm over the last axis; for a row-sharded operator the vectors are row shards and the sum of squares
    is completed over the row group."""
    op, _ = as_operator(matvec)
    if isinstance(op, RowShardedOp):
        from .distributed import sharded_norm

        return sharded_norm(op.comm, V)
    return torch.linalg.vector_norm(V, dim=-1)


def tridiag(matvec, krylov_depth, /, *, reortho: str, custom_vjp: bool = True):
    if reortho == "full":
        return _tridiag_reortho_full(matvec, krylov_depth, custom_vjp=custom_vjp)
    if reortho == "none":
        return _tridiag_reortho_none(matvec, krylov_depth, custom_vjp=custom_vjp)

    msg = f"reortho={reortho} unsupported. Choose eiter {'full', 'none'}."
    raise ValueError(msg)


def _tridiag_reortho_full(matvec, krylov_depth, /, *, custom_vjp):
    # lanczos.py:152-169: Arnoldi with full re-orthogonalisation, then symmetrise H.
    alg = arnoldi.hessenberg(matvec, krylov_depth, custom_vjp=custom_vjp, reortho="full")

    def estimate(vec, *params):
        Q, H, v, _norm = alg(vec, *params)
        T = 0.5 * (H + H.transpose(-1, -2))
        diags = torch.diagonal(T, 0, -2, -1)
        offdiags = torch.diagonal(T, 1, -2, -1)
        vnorm = _vec_norm(v, matvec) if v.dim() == 2 else _vec_norm(v[None], matvec)[0]
        decomposition = (Q.transpose(-1, -2), (diags, offdiags))
        remainder = (v / vnorm[..., None], vnorm)
        return decomposition, remainder

    return estimate


def _tridiag_reortho_none(matvec, krylov_depth, /, *, custom_vjp):
    op, bound = as_operator(matvec)
    sharded = isinstance(op, RowShardedOp)
    k = int(krylov_depth)

    def estimate(vec, *params):
        if bound is not None:
            params = tuple(bound) + tuple(params)
        batched = vec.dim() == 2
        V = vec if batched else vec[None]
        n = op.comm.n if sharded else V.shape[-1]
        if sharded and V.shape[-1] != op.comm.nrows:
            raise ValueError(f"row-sharded operator: expected this rank's {op.comm.nrows} rows of the start vector, got {V.shape[-1]}")
        if k < 1 or k > n:
            raise ValueError(f"Parameter depth {k} is outside the expected range")
        wants_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (V, *params, *differentiable_inputs(op)))
        if not sharded and not custom_vjp and wants_grad:  # autodiff through the loop (the reference's baseline), see _autodiff.py
            from . import _autodiff

            xs, alpha, beta = _autodiff.batched(_autodiff.lanczos_forward, V, op, k, params)
        else:  # (a row-sharded operator: vectors are row shards, alpha / beta replicated)
            cparams = op.constrain(*params)
            xs, alpha, beta = _LanczosFn.apply(op, k, custom_vjp, V, *cparams)
        out = (xs[:, :-1], (alpha, beta[:, :-1])), (xs[:, -1], beta[:, -1])
        if not batched:
            out = (out[0][0][0], (out[0][1][0][0], out[0][1][1][0])), (out[1][0][0], out[1][1][0])
        return out

    return estimate


class _LanczosFn(torch.autograd.Function):
    """``mfx_lanczos_forward`` / ``mfx_lanczos_adjoint``, and for a row-sharded operator their ``_sharded`` forms: V, xs, dv then hold
    this rank's rows; alpha, beta are replicated; the parameter gradients are summed over the row group before they are returned."""

    @staticmethod
    def forward(ctx, op, k, differentiable, V, *cparams):
        tensors = stash_params(ctx, cparams)
        _lib.require_device(V, *tensors)
        lib = _lib.get()
        V = V.contiguous()
        p, nrows = V.shape
        sharded = isinstance(op, RowShardedOp)
        n = op.comm.n if sharded else nrows
        dt, dev = V.dtype, V.device
        xs = torch.empty((p, k + 1, nrows), dtype=dt, device=dev)
        alpha = torch.empty((p, k), dtype=dt, device=dev)
        beta = torch.empty((p, k), dtype=dt, device=dev)
        vnorm = torch.empty((p,), dtype=dt, device=dev)
        call = DriverCall(op, cparams, dt, n)
        if sharded:
            ws = call.take(lib.mfx_sharded_workspace_bytes, n, k, p, device=dev, visible=(xs,))
        else:
            ws = call.take(lib.mfx_workspace_bytes, n, k, p, device=dev, visible=(V, xs))
        call.run(lib.mfx_lanczos_forward_sharded if sharded else lib.mfx_lanczos_forward, _lib.ptr(V), n, k, p, _lib.ptr(xs),
                 _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(vnorm), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        ctx.op, ctx.k, ctx.differentiable = op, k, differentiable
        ctx.save_for_backward(xs, alpha, beta, vnorm, *tensors)
        ctx.set_materialize_grads(False)
        return xs, alpha, beta

    @staticmethod
    def backward(ctx, dxs, dalpha, dbeta):
        if not ctx.differentiable:
            raise RuntimeError("tridiag(custom_vjp=False) is not differentiable in the MI355X build; "
                               "use custom_vjp=True (the adjoint system).")
        xs, alpha, beta, vnorm, *tensors = ctx.saved_tensors
        cparams = rebuild_params(ctx, tensors)
        op, k, lib = ctx.op, ctx.k, _lib.get()
        p, _, nrows = xs.shape
        sharded = isinstance(op, RowShardedOp)
        n = op.comm.n if sharded else nrows
        dt, dev = xs.dtype, xs.device
        dxs = None if dxs is None else dxs.contiguous()
        dalpha = torch.zeros_like(alpha) if dalpha is None else dalpha.contiguous()
        dbeta = torch.zeros_like(beta) if dbeta is None else dbeta.contiguous()
        # no cotangent wanted for the start vector: the driver skips what only produces it (dv == NULL, include/mfx.h)
        dv = torch.empty((p, nrows), dtype=dt, device=dev) if ctx.needs_input_grad[3] else None
        Lam = torch.empty((p, k, nrows), dtype=dt, device=dev)
        call = DriverCall(op, cparams, dt, n, want_grads=True)
        if sharded:
            Lamfull = torch.empty((p, k, n), dtype=dt, device=dev)
            ws = call.take(lib.mfx_sharded_workspace_bytes, n, k, p, device=dev, visible=(Lam, Lamfull))
            entry, gathered = lib.mfx_lanczos_adjoint_sharded, (_lib.ptr(Lamfull),)
        else:
            ws = call.take(lib.mfx_workspace_bytes, n, k, p, device=dev, visible=(xs, Lam, dv, dxs))
            entry, gathered = lib.mfx_lanczos_adjoint, ()
        call.run(entry, n, k, p, _lib.ptr(xs), _lib.ptr(alpha), _lib.ptr(beta), _lib.ptr(vnorm), _lib.ptr(dxs), _lib.ptr(dalpha),
                 _lib.ptr(dbeta), _lib.ptr(dv), _lib.ptr(Lam), *gathered, call.gptr, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        if sharded:
            reduce_grads_(op.comm, call.grads)
        return (None, None, None, dv, *call.grads)


# ------------------------------------------------------------------------------------------------
# k x k eigen-problem of the tridiagonal and the quadrature e1^T f(T) e1  (lanczos.py:48-59)
# ------------------------------------------------------------------------------------------------
class _QuadformFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, matfun, diag, off):
        evals, evecs = _tridiag_eigh(diag, off)
        with torch.enable_grad():
            lam = evals.detach().requires_grad_(True)
            fx = matfun(lam)  # vmap(matfun)(eigvals), lanczos.py:58
            (dfx,) = torch.autograd.grad(fx.sum(), lam)
        fx = fx.detach()
        value = (evecs[:, 0, :] ** 2 * fx).sum(-1)
        ctx.save_for_backward(evals, evecs, fx, dfx)
        ctx.mark_non_differentiable(evals, evecs)
        return value, evals, evecs

    @staticmethod
    def backward(ctx, gout, _dvals, _dvecs):
        evals, evecs, fx, dfx = ctx.saved_tensors
        lib = _lib.get()
        p, k = evals.shape
        dt, dev = evals.dtype, evals.device
        gout = gout.contiguous()
        dalpha = torch.empty((p, k), dtype=dt, device=dev)
        dbeta = torch.empty((p, max(k - 1, 1)), dtype=dt, device=dev)
        _lib.check(lib.mfx_slq_quadform_bwd(_lib.ptr(evals), _lib.ptr(evecs), _lib.ptr(fx), _lib.ptr(dfx.contiguous()),
                                            _lib.ptr(gout), p, k, _lib.dtype_code(dt), _lib.ptr(dalpha),
                                            _lib.ptr(dbeta), max(k - 1, 1), _lib.stream_ptr(dev)))
        return None, dalpha, dbeta[:, : k - 1]


def _flatten(v0):
    """jax.flatten_util.ravel_pytree for (nested) tuples/lists/dicts of tensors (lanczos.py:24)."""
    if torch.is_tensor(v0):
        return v0, None
    leaves, spec = [], []

    def rec(t):
        if torch.is_tensor(t):
            leaves.append(t)
            return ("leaf", t.shape)
        if isinstance(t, dict):
            return ("dict", [(key, rec(t[key])) for key in sorted(t)])
        if isinstance(t, (tuple, list)):
            return (type(t).__name__, [rec(s) for s in t])
        raise TypeError(f"unsupported pytree node {type(t)}")

    spec = rec(v0)
    flat = torch.cat([leaf.reshape(-1) for leaf in leaves])

    def unflatten(f):
        pos = [0]

        def build(s):
            kind, payload = s
            if kind == "leaf":
                num = int(torch.Size(payload).numel())
                out = f[pos[0] : pos[0] + num].reshape(payload)
                pos[0] += num
                return out
            if kind == "dict":
                return {key: build(sub) for key, sub in payload}
            seq = [build(sub) for sub in payload]
            return tuple(seq) if kind == "tuple" else seq

        return build(spec)

    return flat, unflatten


def _flat_matvec(matvec, unflatten):
    if unflatten is None:
        return matvec
    op, bound = as_operator(matvec)
    if not isinstance(op, CallbackOp):
        raise TypeError("pytree start vectors need a Python-callable matvec")

    def matvec_flat(v_flat, *p):
        av = op.fn(unflatten(v_flat), *p)
        return _flatten(av)[0]

    return CallbackOp(matvec_flat) if bound is None else CallbackOp(matvec_flat).bind(*bound)


def integrand_spd(matfun, krylov_depth, matvec, /, *, reortho: str = "full",
                  use_adjoints_for_tridiag: bool = True):
    def quadform(v0, *parameters):
        v0_flat, unflatten = _flatten(v0)
        batched = v0_flat.dim() == 2
        V = v0_flat if batched else v0_flat[None]
        # built first: it refuses an operator it cannot take before the norm below enters a collective on a row-sharded one
        algorithm = tridiag(_flat_matvec(matvec, unflatten), krylov_depth,
                            custom_vjp=use_adjoints_for_tridiag, reortho=reortho)
        scale = _vec_norm(V, matvec)
        V = V / scale[:, None]
        (_basis, (diag, off_diag)), _remainder = algorithm(V, *parameters)
        value, _evals, _evecs = _QuadformFn.apply(matfun, diag, off_diag)
        out = scale**2 * value
        return out if batched else out[0]

    quadform.batched = True
    return quadform


# ------------------------------------------------------------------------------------------------
# vector-valued matrix functions  f(A) v ~ |v| Q f(T) e1  (no counterpart in the reference)
# ------------------------------------------------------------------------------------------------
def _tridiag_eigh(diag, off):
    """``mfx_tridiag_eigh`` of the (p, k) / (p, k - 1) tridiagonal, detached: evals (p, k), evecs (p, k, k) in the input dtype."""
    _lib.require_device(diag, off)
    lib = _lib.get()
    diag, off = diag.detach().contiguous(), off.detach().contiguous()
    p, k = diag.shape
    dt, dev = diag.dtype, diag.device
    # beyond depth 120 the eigensolver accumulates its rotations in the fp64 output itself (include/mfx.h): fp32 problems are cast
    et = torch.float64 if k > 120 else dt
    diag_e, off_e = diag.to(et), off.to(et)
    evals = torch.empty((p, k), dtype=et, device=dev)
    evecs = torch.empty((p, k, k), dtype=et, device=dev)
    _lib.check(lib.mfx_tridiag_eigh(_lib.ptr(diag_e), _lib.ptr(off_e) if k > 1 else None, max(k - 1, 1), p, k,
                                    _lib.dtype_code(et), _lib.ptr(evals), _lib.ptr(evecs), _lib.stream_ptr(dev)))
    return evals.to(dt), evecs.to(dt)


class _FunmFn(torch.autograd.Function):
    """y = sum_j c_j q_j with c = scale U (fvals o U[0])  (``mfx_funm_coeffs``, ``mfx_basis_combine``) and its VJP w.r.t. the basis, the
    tridiagonal, the scale and ``fvals`` (``mfx_basis_combine_bwd``, ``mfx_funm_coeffs_bwd``).  ``evals`` / ``evecs`` are the detached
    eigen-problem of (diag, off) and ``dfvals`` = f'(evals): the dependence of the eigen-problem on the tridiagonal is what the
    divided-difference VJP accounts for.  ``fvals`` is an input of its own so that gradients reach whatever ``matfun`` closes over."""

    @staticmethod
    def forward(ctx, Q, diag, off, scale, evals, evecs, fvals, dfvals):
        _lib.require_device(Q, diag, off, scale, evals, evecs, fvals, dfvals)
        lib = _lib.get()
        Q = Q.contiguous()
        p, k, n = Q.shape
        dt, dev = Q.dtype, Q.device
        code = _lib.dtype_code(dt)
        scale, evals, evecs = scale.contiguous(), evals.contiguous(), evecs.contiguous()
        fvals, dfvals = fvals.to(dt).contiguous(), dfvals.to(dt).contiguous()
        coeffs = torch.empty((p, k), dtype=dt, device=dev)
        y = torch.empty((p, n), dtype=dt, device=dev)
        _lib.check(lib.mfx_funm_coeffs(_lib.ptr(evals), _lib.ptr(evecs), _lib.ptr(fvals), _lib.ptr(scale), p, k, code,
                                       _lib.ptr(coeffs), _lib.stream_ptr(dev)))
        _lib.check(lib.mfx_basis_combine(_lib.ptr(Q), _lib.ptr(coeffs), n, k, p, code, _lib.ptr(y), _lib.stream_ptr(dev)))
        ctx.save_for_backward(Q, coeffs, scale, evals, evecs, fvals, dfvals)
        return y

    @staticmethod
    def backward(ctx, dy):
        Q, coeffs, scale, evals, evecs, fvals, dfvals = ctx.saved_tensors
        lib = _lib.get()
        p, k, n = Q.shape
        dt, dev = Q.dtype, Q.device
        code = _lib.dtype_code(dt)
        dy = dy.contiguous()
        need_q = ctx.needs_input_grad[0]
        need_c = any(ctx.needs_input_grad[i] for i in (1, 2, 3, 6))
        if not (need_q or need_c):
            return (None,) * 8
        dQ = torch.empty((p, k, n), dtype=dt, device=dev) if need_q else None
        dcoeffs = torch.empty((p, k), dtype=dt, device=dev) if need_c else None
        ws = _lib.scratch(int(lib.mfx_basis_combine_workspace_bytes(n, k, p, code)), dev)
        _lib.check(lib.mfx_basis_combine_bwd(_lib.ptr(Q), _lib.ptr(coeffs), _lib.ptr(dy), n, k, p, code, _lib.ptr(dQ),
                                             _lib.ptr(dcoeffs), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        dalpha = dbeta = dscale = dfv = None
        if need_c:
            dalpha = torch.empty((p, k), dtype=dt, device=dev)
            dbeta = torch.empty((p, max(k - 1, 1)), dtype=dt, device=dev)
            dscale = torch.empty((p,), dtype=dt, device=dev)
            _lib.check(lib.mfx_funm_coeffs_bwd(_lib.ptr(evals), _lib.ptr(evecs), _lib.ptr(fvals), _lib.ptr(dfvals), _lib.ptr(dcoeffs),
                                               _lib.ptr(scale), p, k, code, _lib.ptr(dalpha), _lib.ptr(dbeta), max(k - 1, 1),
                                               _lib.ptr(dscale), _lib.stream_ptr(dev)))
            dbeta = dbeta[:, : k - 1]
            if ctx.needs_input_grad[6]:  # d fvals[b][a] = scale (U^T dc)_a u0_a: (p, k, k) plumbing, only when matfun's closure wants it
                dfv = scale[:, None] * torch.einsum("pja,pj->pa", evecs, dcoeffs) * evecs[:, 0, :]
        return dQ, dalpha, dbeta, dscale, None, None, dfv, None


def _funm_apply(matfun, Q, diag, off, scale):
    """scale Q^T f(T) e1 for the (p, k, n) basis and (p, k) / (p, k - 1) tridiagonal of ``tridiag``: eigen-problem on the device, f and f' by
    torch on the (p, k) eigenvalues, coefficients and combination by libmfx."""
    evals, evecs = _tridiag_eigh(diag, off)
    with torch.enable_grad():
        lam = evals.detach().requires_grad_(True)
        (dfx,) = torch.autograd.grad(matfun(lam).sum(), lam, allow_unused=True)
    if dfx is None:
        dfx = torch.zeros_like(evals)
    # A second evaluation on the (p, k) eigenvalues, deliberately: on the DETACHED eigenvalues the values are attached only to what
    # matfun closes over (expm_lanczos: dt).  The values of the evaluation above hang on `lam` as well, so with them _FunmFn would see an
    # input that always requires grad, and every backward would form the fvals cotangent and push it into that throwaway leaf.
    fx = matfun(evals)
    return _FunmFn.apply(Q, diag, off, scale, evals, evecs, fx, dfx)


def funm_spd(matfun, krylov_depth, matvec, /, *, reortho: str = "full", custom_vjp: bool = True):
    """f(A) v ~ |v| Q f(T) e1 for a symmetric operator: ``apply(v, *params) -> f(A) v`` with v (n,) or (p, n).

    ``matfun`` is any torch callable on the (p, k) eigenvalues of the tridiagonal.  Differentiable w.r.t. v, the parameters, the inputs of
    a kernel-Gram operator and whatever ``matfun`` closes over: the VJP of f(T) e1 is in divided-difference form (stable for close Ritz
    values, as ``integrand_spd``'s), and the adjoint drivers of ``tridiag`` turn the basis / tridiagonal cotangents into the rest.
    A row-sharded operator is refused: there is no sharded combination."""

    def apply(v, *parameters):
        op, _ = as_operator(matvec)
        if isinstance(op, RowShardedOp):
            raise NotImplementedError("funm_spd on a row-sharded operator: there is no sharded basis combination")
        batched = v.dim() == 2
        V = v if batched else v[None]
        algorithm = tridiag(matvec, krylov_depth, custom_vjp=custom_vjp, reortho=reortho)  # refusals before any work
        scale = torch.linalg.vector_norm(V, dim=-1)
        V = V / scale[:, None]
        (basis, (diag, off_diag)), _remainder = algorithm(V, *parameters)
        out = _funm_apply(matfun, basis, diag, off_diag, scale)
        return out if batched else out[0]

    apply.batched = True
    return apply


def integrand_spd_custom_vjp_reuse(matfun, order, matvec, /, *, reortho: str = "full"):
    """SLQ integrand whose backward pass re-uses the forward Lanczos basis (lanczos.py:64-139):
    one matvec-VJP, inexact gradient (Dong et al. 2017), first order only, zero gradient w.r.t. v0."""
    op, bound = as_operator(matvec)

    def quadform(v0, *parameters):
        if bound is not None:
            parameters = tuple(bound) + tuple(parameters)
        v0_flat, unflatten = _flatten(v0)
        if unflatten is not None:
            raise TypeError("integrand_spd_custom_vjp_reuse: pytree start vectors are not supported")
        batched = v0_flat.dim() == 2
        V = v0_flat if batched else v0_flat[None]
        out = _ReuseFn.apply(op, matfun, int(order), reortho, len(parameters), V, *parameters, *differentiable_inputs(op))
        return out if batched else out[0]

    quadform.batched = True
    return quadform


class _ReuseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op, matfun, order, reortho, nparams, V, *parameters):
        # parameters: the matvec's nparams parameters, then the tensors the operator closes over (differentiable_inputs)
        parameters = parameters[:nparams]
        with torch.no_grad():
            scale = torch.linalg.vector_norm(V, dim=-1)
            U = V / scale[:, None]
            algorithm = tridiag(op, order, custom_vjp=False, reortho=reortho)
            (basis, (diag, off)), _ = algorithm(U, *parameters)
            value, evals, evecs = _QuadformFn.apply(matfun, diag, off)
            with torch.enable_grad():
                lam = evals.detach().requires_grad_(True)
                (dfx,) = torch.autograd.grad(matfun(lam).sum(), lam)
            sol = torch.einsum("pia,pa->pi", evecs, dfx * evecs[:, 0, :])  # lanczos.py:116
            w1 = scale[:, None] ** 2 * torch.einsum("pin,pi->pn", basis, sol)  # lanczos.py:117
        ctx.op = op
        ctx.nparams = nparams
        ctx.save_for_backward(w1, U, *stash_params(ctx, (*parameters, *differentiable_inputs(op))))
        return scale**2 * value

    @staticmethod
    def backward(ctx, gout):
        w1, w2, *tensors = ctx.saved_tensors
        params = rebuild_params(ctx, tensors)
        warnings.warn("Todo: implement gradient wrt v correctly", stacklevel=1)  # lanczos.py:131-133
        with torch.enable_grad():
            live = [q.detach().requires_grad_(True) if torch.is_tensor(q) and q.is_floating_point() else q for q in params]
            diff = [q for q in live if torch.is_tensor(q) and q.requires_grad]
            op = with_inputs(ctx.op, live[ctx.nparams:])  # (the inputs X of a kernel-Gram operator, when they need a gradient)
            fx = (op(w2, *live[: ctx.nparams]) * w1 * gout[:, None]).sum()  # (A(p) w2)^T w1, lanczos.py:128
            grads = torch.autograd.grad(fx, diff, allow_unused=True)
        it = iter(grads)
        out = [next(it) if (torch.is_tensor(q) and q.requires_grad) else None for q in live]
        return (None, None, None, None, None, torch.zeros_like(w2), *out)
