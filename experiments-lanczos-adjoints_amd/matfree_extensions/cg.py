"""Conjugate gradient solvers -- MI355X build.

Same functional surface as the reference's ``matfree_extensions/cg.py``:

    cg_fixed_step(num_matvecs)(A, b)                         pcg_fixed_step(num_matvecs)(A, b, P)
    cg_adaptive(atol=, rtol=, maxiter=, miniter=)(A, b)      pcg_adaptive(...)(A, b, P)
        -> (x, info)   info = {"residual_abs", "residual_rel"[, "num_steps"]}

with the whole iteration (cg.py:27-58, 85-135) executed by libmfx (``mfx_pcg_solve``).  ``A`` is a native operator
(``op.bind(*params)``) or any callable ``A(v)``; ``b`` may be a batch (p, n) of right-hand sides (each is solved
independently, adaptive stopping included).  ``P`` is ``low_rank.Preconditioner.bind(s)`` (or ``None``): arbitrary Python
preconditioners are not supported inside the HIP loop.  ``A`` may be an ``operators.RowShardedOp`` (bound): ``b``, ``x`` and the
residuals are then this rank's rows, ``P`` is the same (replicated) preconditioner object on every rank -- its rows are taken
here -- and the loop runs in ``mfx_pcg_solve_sharded`` (not for the re-orthogonalising variant).

Differentiation is the rule of ``jax.lax.custom_linear_solve(..., symmetric=True)`` (cg.py:23-25): the cotangent of the
right-hand side is another solve with the same solver, the cotangent of the operator's parameters is the parameter sweep
with (-lambda, x); nothing flows through the preconditioner or the info dict.

    mbcg_fixed_step(num_matvecs)(A, b, P)        mbcg_adaptive(atol=, rtol=, maxiter=, miniter=)(A, b, P)
        -> (x, info)   info = {"residual_abs", "num_steps", "tridiag": (diag, offdiag), "rz0", "depth", "w0"}

are the same solves (``x``, the residual and the step counts are ``pcg_*``'s bit for bit, ``x`` differentiable in the same way)
through ``mfx_mbcg_solve``, which also keeps the CG coefficients: per right-hand side the Lanczos tridiagonal of the preconditioned
system, padded with an identity block beyond ``depth`` (include/mfx.h).  ``util.gp_util.krylov_logdet_mbcg`` / ``logpdf_mbcg`` turn
them into the log-determinant and the GP log-likelihood.  Not row-sharded.  ``cg_fixed_step_reortho`` /
``pcg_fixed_step_reortho`` (cg.py:140-219; "needs more work" according to the reference's own test) are reproduced as they are.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .low_rank import BoundPreconditioner
from .operators import CallbackOp, DriverCall, RowShardedOp, as_operator, rebuild_params, reduce_grads_, stash_params


def cg_fixed_step(*args, **kwargs):
    pcg_solve = pcg_fixed_step(*args, **kwargs)

    def cg(A, b):
        return pcg_solve(A, b, None)

    return cg


def pcg_fixed_step(num_matvecs: int, /):
    cfg = {"maxiter": int(num_matvecs), "miniter": 0, "atol": 1.0, "rtol": 0.0, "adaptive": False}

    def pcg(A, b, P):
        x, r, _steps = _solve(A, b, P, cfg)
        return x, {"residual_abs": r, "residual_rel": r / x.detach().abs()}

    return pcg


def cg_fixed_step_reortho(*args, **kwargs):
    pcg_solve = pcg_fixed_step_reortho(*args, **kwargs)

    def cg(A, b):
        return pcg_solve(A, b, None)

    return cg


def pcg_fixed_step_reortho(num_matvecs: int, /):
    """cg.py:151-219: every step re-orthogonalises the residual against the stored normalised residuals Q."""
    cfg = {"maxiter": int(num_matvecs), "miniter": 0, "atol": 1.0, "rtol": 0.0, "adaptive": False, "reortho": True}

    def pcg(A, b, P):
        x, r, Q = _solve(A, b, P, cfg)
        return x, {"residual_abs": r, "Q": Q.transpose(-1, -2)}

    return pcg


def cg_adaptive(**kwargs):
    pcg_solve = pcg_adaptive(**kwargs)

    def cg(A, b):
        return pcg_solve(A, b, None)

    return cg


def pcg_adaptive(*, atol: float, rtol, maxiter: int, miniter: int = 0):
    """atol and rtol follow allclose logic (cg.py:73-74)."""
    cfg = {"maxiter": int(maxiter), "miniter": int(miniter), "atol": float(atol), "rtol": float(rtol), "adaptive": True}

    def pcg(A, b, P):
        x, r, steps = _solve(A, b, P, cfg)
        return x, {"residual_abs": r, "residual_rel": r / x.detach().abs(), "num_steps": steps}

    return pcg


def mbcg_fixed_step(num_matvecs: int, /):
    """pcg_fixed_step that keeps its coefficients (modified batched CG): see the module docstring."""
    cfg = {"maxiter": int(num_matvecs), "miniter": 0, "atol": 1.0, "rtol": 0.0, "adaptive": False, "mbcg": True}

    def mbcg(A, b, P):
        return _mbcg(A, b, P, cfg)

    mbcg.cfg = cfg
    return mbcg


def mbcg_adaptive(*, atol: float, rtol, maxiter: int, miniter: int = 0):
    """pcg_adaptive that keeps its coefficients (modified batched CG): see the module docstring."""
    cfg = {"maxiter": int(maxiter), "miniter": int(miniter), "atol": float(atol), "rtol": float(rtol), "adaptive": True,
           "mbcg": True}

    def mbcg(A, b, P):
        return _mbcg(A, b, P, cfg)

    mbcg.cfg = cfg
    return mbcg


def _mbcg(A, b, P, cfg):
    x, r, steps, diag, off, rz0, depth, w0 = _solve(A, b, P, cfg)
    return x, {"residual_abs": r, "num_steps": steps, "tridiag": (diag, off), "rz0": rz0, "depth": depth, "w0": w0}


def _check_mbcg(op, P, cfg):
    if cfg["maxiter"] < 1:
        raise ValueError("mBCG needs at least one iteration (num_matvecs / maxiter >= 1)")
    if isinstance(op, RowShardedOp):
        raise NotImplementedError("mBCG is not row-sharded in the MI355X build (mfx_mbcg_solve has no sharded form); shard the "
                                  "probes instead of the rows")
    if P is not None and not isinstance(P, BoundPreconditioner):
        raise TypeError("P must be None or low_rank.Preconditioner.bind(s): the PCG loop runs inside libmfx and "
                        "cannot call back into an arbitrary Python preconditioner")


def _solve(A, b, P, cfg):
    op, bound = as_operator(A)
    if cfg.get("mbcg", False):
        _check_mbcg(op, P, cfg)
    if isinstance(op, RowShardedOp) and cfg.get("reortho", False):
        raise NotImplementedError("the re-orthogonalising PCG variant is not row-sharded in the MI355X build")
    params = tuple(bound) if bound is not None else ()
    if P is not None and not isinstance(P, BoundPreconditioner):
        raise TypeError("P must be None or low_rank.Preconditioner.bind(s): the PCG loop runs inside libmfx and "
                        "cannot call back into an arbitrary Python preconditioner")
    batched = b.dim() == 2
    B = b if batched else b[None]
    cparams = op.constrain(*params)
    out = _PcgFn.apply(op, cfg, P, B, *cparams)  # (x, r, steps[, mBCG extras]); steps: int64 (p,), or the basis Q (p, m, n) when re-orthogonalising
    if not batched:
        return tuple(t[0] for t in out)
    return out


def _precond(P, n, dtype, cols=None):
    """-> (rank, lt, minv, shift) of the bound preconditioner ``P`` (None: none) for a system of size n; ``cols``: the columns of
    L^T of a row shard."""
    if P is None:
        return 0, None, None, None
    pre = P.pre
    if pre.n != n or pre.lt.dtype != dtype:
        raise ValueError(f"preconditioner of size {pre.n} ({pre.lt.dtype}) used for a system of size {n} ({dtype})")
    lt = pre.lt if cols is None else pre.lt[:, cols].contiguous()  # this rank's columns of L^T
    minv, shift = pre.minv(P.s)  # from the whole L: replicated
    return pre.rank, lt, minv, shift


def _run(op, cfg, P, B, cparams):
    """One mfx_pcg_solve (row-sharded operator: mfx_pcg_solve_sharded, with B, x, r this rank's rows and steps replicated),
    mfx_pcg_solve_reortho or mfx_mbcg_solve call on detached tensors -> (x, r, steps), (x, r, Q) or
    (x, r, steps, tdiag, toff, rz0, depth, w0); the padded tridiagonals are (p, maxiter) each."""
    lib = _lib.get()
    sharded = isinstance(op, RowShardedOp)
    B = B.contiguous()
    p, nrows = B.shape
    n = op.comm.n if sharded else nrows
    if sharded and nrows != op.comm.nrows:
        raise ValueError(f"row-sharded operator: expected this rank's {op.comm.nrows} rows of the right-hand side, got {nrows}")
    dt, dev = B.dtype, B.device
    call = DriverCall(op, cparams, dt, n)
    rank, lt, minv, shift = _precond(P, n, dt, slice(op.comm.row0, op.comm.row0 + op.comm.nrows) if sharded else None)
    m, reortho, mbcg = cfg["maxiter"], cfg.get("reortho", False), cfg.get("mbcg", False)
    if mbcg:
        ws = call.take(lib.mfx_mbcg_workspace_bytes, n, p, rank, m, device=dev)
    elif sharded:
        ws = call.take(lib.mfx_pcg_sharded_workspace_bytes, n, p, rank, device=dev)
    else:
        ws = call.take(lib.mfx_pcg_workspace_bytes, n, p, max(rank, m) if reortho else rank, device=dev)
    x = torch.empty_like(B)
    r = torch.empty_like(B)
    system = (_lib.ptr(B), nrows, n, p, _lib.ptr(lt), rank, _lib.ptr(minv), _lib.ptr(shift))
    stop = (m, cfg["miniter"], cfg["atol"], cfg["rtol"], int(cfg["adaptive"]))
    tail = (_lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    if reortho:
        if m < 1:
            raise ValueError("pcg_fixed_step_reortho needs num_matvecs >= 1")
        Q = torch.zeros((p, m, n), dtype=dt, device=dev)
        call.run(lib.mfx_pcg_solve_reortho, *system, m, _lib.ptr(x), _lib.ptr(r), _lib.ptr(Q), *tail)
        return x, r, Q
    steps = torch.empty((p,), dtype=torch.int64, device=dev)
    if mbcg:
        depth = torch.empty((p,), dtype=torch.int64, device=dev)
        tdiag = torch.empty((p, m), dtype=dt, device=dev)
        toff = torch.empty((p, m), dtype=dt, device=dev)
        rz0 = torch.empty((p,), dtype=dt, device=dev)
        w0 = torch.empty_like(B)
        call.run(lib.mfx_mbcg_solve, *system, *stop, _lib.ptr(x), _lib.ptr(r), _lib.ptr(steps), _lib.ptr(w0), _lib.ptr(tdiag),
                 _lib.ptr(toff), _lib.ptr(rz0), _lib.ptr(depth), *tail)
        return x, r, steps, tdiag, toff, rz0, depth, w0
    call.run(lib.mfx_pcg_solve_sharded if sharded else lib.mfx_pcg_solve, *system, *stop, _lib.ptr(x), _lib.ptr(r), _lib.ptr(steps),
             *tail)
    return x, r, steps


class _PcgFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op, cfg, P, B, *cparams):
        tensors = stash_params(ctx, cparams)
        _lib.require_device(B, *tensors)
        x, *rest = _run(op, cfg, P, B, cparams)
        ctx.op, ctx.P = op, P
        ctx.cfg = {k: v for k, v in cfg.items() if k != "mbcg"}  # the transpose solve needs no coefficients
        ctx.save_for_backward(x, *tensors)
        ctx.mark_non_differentiable(*rest)
        return (x, *rest)

    @staticmethod
    def backward(ctx, dx, *_unused):
        x, *tensors = ctx.saved_tensors
        cparams = rebuild_params(ctx, tensors)
        op = ctx.op
        lam, _r, _s = _run(op, ctx.cfg, ctx.P, dx, cparams)  # symmetric=True: the transpose solve is the same solve
        p, nrows = x.shape
        if isinstance(op, CallbackOp):
            grads = []
            diff_idx = [i for i, q in enumerate(cparams) if torch.is_tensor(q) and q.is_floating_point()]
            acc = {i: torch.zeros_like(cparams[i]) for i in diff_idx}
            for bidx in range(p):
                with torch.enable_grad():
                    live = [q.detach().requires_grad_(True) if i in acc else q for i, q in enumerate(cparams)]
                    diff = [live[i] for i in diff_idx]
                    if diff:
                        out = op.fn(x[bidx].detach(), *live)
                        gs = torch.autograd.grad(out, diff, -lam[bidx], allow_unused=True)
                        for i, g in zip(diff_idx, gs):
                            if g is not None:
                                acc[i].add_(g)
            grads = [acc.get(i) for i in range(len(cparams))]
        else:
            sharded = isinstance(op, RowShardedOp)
            nat, n = (op.op, op.comm.n) if sharded else (op, nrows)
            desc = nat.descriptor(cparams, x.dtype, n)
            if sharded:  # this rank's rows of -lambda against ALL entries of x; partial sums -> one all-reduce
                desc.row0, desc.nrows = op.comm.row0, op.comm.nrows
            gstruct, grads = nat.new_grads(*cparams)
            ws = _lib.workspace(desc, n, 1, p, x.device)
            L = (-lam).contiguous()
            R = op.comm.gather_rows(x) if sharded else x
            _lib.check(_lib.get().mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), nrows, _lib.ptr(R), n, p, C.byref(gstruct),
                                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
            if sharded:
                reduce_grads_(op.comm, grads)
        return (None, None, None, lam, *grads)
