"""PDE matrix-function helpers on the Arnoldi path -- MI355X build ("next" tier).

Covers the pieces of the reference's ``util/pde_util.py`` that are thin compositions of the hot path:
``expm_arnoldi`` (:257-268), its dense baseline ``expm_pade`` (:271-280), ``solver_expm`` (:240-252), ``sampler_lanczos`` (:335-356),
the small helpers ``mesh_tensorproduct`` / ``loss_mse`` / ``loss_mse_relative`` (:14-15, :160-173) and the 5-point wave operator
(:18-20,126-157) expressed as a native CSR operator so that the non-symmetric Arnoldi forward/adjoint kernels run it
end to end.  The dense k x k ``expm`` / ``eigh`` are torch calls (k <= ~100: plumbing, differentiable).

The reference's stencil vector fields themselves -- ``pde_heat`` / ``pde_heat_affine`` / ``pde_heat_anisotropic`` /
``pde_wave_anisotropic`` with ``boundary_dirichlet`` / ``boundary_neumann`` and any 3x3 stencil (:18-157) -- run matrix-free on
``operators.StencilOp``; ``wave_operator`` (the assembled CSR form of one of them) stays.

The fixed-step Runge-Kutta baselines of the work-precision study (``solver_euler`` / ``solver_diffrax``, :177-237) are ``solver_rk``:
the whole solve, its discrete adjoint and the continuous ("backsolve") adjoint are single libmfx driver calls (``mfx_rk_solve`` /
``mfx_rk_adjoint`` / ``mfx_rk_backsolve``, csrc/mfx_rk.hip) on LINEAR autonomous fields y' = A y, A a native, bound or callback
operator.  AFFINE fields y' = A y + b go through ``operators.AffineOp``, the bordered linear operator on (y, 1): ``rhs.flat`` of
``pde_heat_affine`` is one, and ``solver_expm`` / ``solver_rk`` / ``solver_euler`` lift the state, solve and drop the last entry.
ADAPTIVE steps are ``solver_rk_adaptive``: an embedded pair under scipy's step-size controller, the step size held on the device
(``mfx_rk_solve_adaptive``), gradients by the fixed-step adjoints on the accepted steps.
Out of scope: nonlinear fields, gradients with respect to the times, row-sharded operators.
"""

from __future__ import annotations

import numpy as np
import torch

import ctypes as C

from .. import _lib, arnoldi, lanczos
from ..operators import (AffineOp, BoundOp, CallbackOp, CsrOp, DriverCall, NativeOp, RbfGramOp, RowShardedOp, StencilOp, as_operator, rebuild_params,
                         stash_params)
from . import rk_tableaux


def expm_arnoldi(krylov_depth, *, max_squarings: int = 32, reortho="full", custom_vjp=True):
    """exp(dt A) y0 ~ (1/c) Q expm(dt H) e1  (util/pde_util.py:257-268).  ``max_squarings`` is accepted for signature
    parity (torch.linalg.matrix_exp chooses its own scaling)."""

    def expm(matvec, dt, y0_flat, *p):
        algorithm = arnoldi.hessenberg(matvec, krylov_depth, reortho=reortho, custom_vjp=custom_vjp)
        Q, H, _r, c = algorithm(y0_flat, *p)
        op, _ = as_operator(matvec)
        if isinstance(op, RowShardedOp):  # y0, Q and the result are row shards; H and c are replicated but consumed per shard
            from ..distributed import sum_grad

            H, c = sum_grad(op.comm, H), sum_grad(op.comm, c)
        expmat = torch.linalg.matrix_exp(dt * H)
        # Q expm(dt H) e1 as a weighted sum over the (k, n) storage of the basis: elementwise kernels in both directions (as a
        # matmul on the transposed view the backward went to a 41 ms skinny rocBLAS GEMM at n = 2e6)
        Qkn = Q.transpose(-1, -2)
        out = (Qkn * expmat[..., :, 0:1]).sum(dim=-2) / (c[..., None] if c.dim() else c)
        return out, {"num_matvecs": krylov_depth}

    return expm


def expm_lanczos(krylov_depth, *, reortho="full", custom_vjp=True):
    """exp(dt A) y0 ~ |y0| Q exp(dt T) e1 for a SYMMETRIC operator, with expm_arnoldi's call signature.  The k x k exponential is the
    eigen-decomposition of the tridiagonal on the device and the combination over the basis is one native pass (``lanczos.funm_spd``);
    the backward is the divided-difference VJP, not autograd through ``eigh`` / ``matrix_exp``.  ``dt`` may be a tensor that requires
    grad.  No counterpart in the reference; expm_arnoldi is unchanged."""

    def expm(matvec, dt, y0_flat, *p):
        apply = lanczos.funm_spd(lambda lam: torch.exp(dt * lam), krylov_depth, matvec, reortho=reortho, custom_vjp=custom_vjp)
        return apply(y0_flat, *p), {"num_matvecs": krylov_depth}

    return expm


def expm_pade():
    """Dense baseline of expm_arnoldi (util/pde_util.py:271-280): materialise A through the matvec (the reference takes its Jacobian; the
    matvec is linear, so n applications to the identity are the same matrix) and apply torch.linalg.matrix_exp(dt A) to y0.  Small n only."""

    def expm(matvec, dt, y0_flat, *p):
        n = y0_flat.shape[0]
        op, _ = as_operator(matvec)
        cols = op(torch.eye(n, dtype=y0_flat.dtype, device=y0_flat.device), *p)  # row b = A e_b
        return torch.linalg.matrix_exp(dt * cols.t()) @ y0_flat

    return expm


def mesh_tensorproduct(x, y, /):
    """util/pde_util.py:14-15: jnp.stack(jnp.meshgrid(x, y)) -- 'xy' indexing, shape (2, len(y), len(x))."""
    return torch.stack(torch.meshgrid(x, y, indexing="xy"))


def loss_mse():
    """util/pde_util.py:160-164."""

    def loss(sol, /, *, targets):
        return torch.mean((sol - targets) ** 2)

    return loss


def loss_mse_relative(*, nugget, reduce=torch.mean):
    """util/pde_util.py:167-173."""

    def loss(sol, /, *, targets):
        mse_abs = (sol - targets) ** 2
        return reduce(mse_abs / (nugget + torch.abs(targets)))

    return loss


def solver_expm(t0, t1, vector_field, /, expm):
    """util/pde_util.py:240-252 for flat states: y(t1) = exp((t1 - t0) A) y0 with A v = vector_field(v, *p).  A native operator or
    a bound one (``rhs.flat`` of the stencil vector fields below) acts on the flattened state and goes to ``expm`` as it is: the
    Krylov loop then applies it natively instead of calling back into Python."""

    affine, bound = as_operator(vector_field) if isinstance(vector_field, (NativeOp, BoundOp)) else (None, None)

    def solve(y0, *p):
        shape = y0.shape
        if isinstance(affine, AffineOp):  # exp(dt B) (y0, 1) = (y(t1), 1) on the bordered operator
            m = affine.size(*affine.constrain(*(bound or ()), *p)) - 1
            out, info = expm(vector_field, t1 - t0, AffineOp.lift(_states_of(y0, m)), *p)
            return AffineOp.drop(out).reshape(shape), info
        if isinstance(vector_field, (NativeOp, BoundOp, RowShardedOp)):
            out, info = expm(vector_field, t1 - t0, y0.reshape(-1), *p)
            return out.reshape(shape), info
        out, info = expm(lambda v, *q: vector_field(v.reshape(shape), *q).reshape(-1), t1 - t0, y0.reshape(-1), *p)
        return out.reshape(shape), info

    return solve


def _states_of(y0, n):
    """y0 as one state (n,) or, with one more dimension than the operator's state, a batch (p, n)."""
    if y0.numel() == n:
        return y0.reshape(n)
    if y0.dim() >= 2 and y0.shape[0] * n == y0.numel():
        return y0.reshape(y0.shape[0], n)
    raise ValueError(f"a state of shape {tuple(y0.shape)} does not match the operator's {n} unknowns")


_RK_ADJOINTS = {"discrete": "discrete", "recursive_checkpoint": "discrete", "direct": "discrete", "backsolve": "backsolve"}


def _dts_array(dts):
    return (C.c_double * len(dts))(*dts)


def _rk_forward(op, cparams, tab, dts, Y0, keep_ys):
    """One mfx_rk_solve call on detached tensors -> (y1 (p, n), ys (p, nsteps + 1, n) or None)."""
    lib = _lib.get()
    Y0 = Y0.contiguous()
    p, n = Y0.shape
    dt, dev = Y0.dtype, Y0.device
    call = DriverCall(op, cparams, dt, n)
    tstruct = rk_tableaux.struct(tab)
    y1 = torch.empty_like(Y0)
    ys = torch.empty((p, len(dts) + 1, n), dtype=dt, device=dev) if keep_ys else None
    ws = call.take(lambda desc: lib.mfx_rk_workspace_bytes(desc, C.byref(tstruct), n, p, 0), device=dev, visible=(Y0, y1, ys))
    call.run(lib.mfx_rk_solve, C.byref(tstruct), _dts_array(dts), len(dts), _lib.ptr(Y0), n, n, p, _lib.ptr(y1), n, _lib.ptr(ys),
             0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return y1, ys


class _RkFn(torch.autograd.Function):
    """``mfx_rk_solve`` with the iterates kept; backward = ``mfx_rk_adjoint``, the exact gradient of the discrete scheme."""

    @staticmethod
    def forward(ctx, op, tab, dts, Y0, *cparams):
        tensors = stash_params(ctx, cparams)
        _lib.require_device(Y0, *tensors)
        y1, ys = _rk_forward(op, cparams, tab, dts, Y0, True)
        ctx.op, ctx.tab, ctx.dts = op, tab, dts
        ctx.save_for_backward(ys, *tensors)
        return y1

    @staticmethod
    def backward(ctx, dy1):
        ys, *tensors = ctx.saved_tensors
        cparams = rebuild_params(ctx, tensors)
        lib, tab, dts = _lib.get(), ctx.tab, ctx.dts
        p, _, n = ys.shape
        dt, dev = ys.dtype, ys.device
        dy1 = dy1.contiguous()
        dy0 = torch.empty_like(dy1) if ctx.needs_input_grad[3] else None  # NULL: the last lambda store is skipped
        call = DriverCall(ctx.op, cparams, dt, n, want_grads=True)
        tstruct = rk_tableaux.struct(tab)
        ws = call.take(lambda desc: lib.mfx_rk_workspace_bytes(desc, C.byref(tstruct), n, p, 1), device=dev, visible=(ys, dy1, dy0))
        call.run(lib.mfx_rk_adjoint, C.byref(tstruct), _dts_array(dts), len(dts), _lib.ptr(ys), n, p, _lib.ptr(dy1), n, _lib.ptr(dy0), n,
                 call.gptr, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        return (None, None, None, dy0, *call.grads)


class _RkBacksolveFn(torch.autograd.Function):
    """``mfx_rk_solve`` keeping only y1; backward = ``mfx_rk_backsolve``, the continuous adjoint integrated backwards from y1."""

    @staticmethod
    def forward(ctx, op, tab, dts, Y0, *cparams):
        tensors = stash_params(ctx, cparams)
        _lib.require_device(Y0, *tensors)
        y1, _ = _rk_forward(op, cparams, tab, dts, Y0, False)
        ctx.op, ctx.tab, ctx.dts = op, tab, dts
        ctx.save_for_backward(y1, *tensors)
        return y1

    @staticmethod
    def backward(ctx, dy1):
        y1, *tensors = ctx.saved_tensors
        cparams = rebuild_params(ctx, tensors)
        lib, tab, dts = _lib.get(), ctx.tab, ctx.dts
        p, n = y1.shape
        dt, dev = y1.dtype, y1.device
        dy1 = dy1.contiguous()
        dy0 = torch.empty_like(dy1) if ctx.needs_input_grad[3] else None
        call = DriverCall(ctx.op, cparams, dt, n, want_grads=True)
        tstruct = rk_tableaux.struct(tab)
        ws = call.take(lambda desc: lib.mfx_rk_workspace_bytes(desc, C.byref(tstruct), n, p, 2), device=dev, visible=(y1, dy1, dy0))
        call.run(lib.mfx_rk_backsolve, C.byref(tstruct), _dts_array(dts), len(dts), _lib.ptr(y1), n, n, p, _lib.ptr(dy1), n, _lib.ptr(dy0),
                 n, call.gptr, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        return (None, None, None, dy0, *call.grads)


def _rk_solver(dts, vector_field, method, adjoint):
    if adjoint not in _RK_ADJOINTS:
        raise ValueError(f"adjoint must be one of {sorted(_RK_ADJOINTS)}, got {adjoint!r}")
    tab = rk_tableaux.get(method)
    dts = tuple(float(d) for d in dts)
    if len(dts) < 1:
        raise ValueError("a Runge-Kutta solve needs at least one step")
    if not isinstance(vector_field, (NativeOp, BoundOp, CallbackOp, RowShardedOp)):
        raise TypeError("solver_rk integrates LINEAR autonomous fields y' = A y: vector_field must be a linear operator -- a native "
                        "operator, op.bind(*params) (rhs.flat of the stencil vector fields) or operators.CallbackOp(fn) -- not a "
                        f"plain callable ({type(vector_field).__name__}); affine fields y' = A y + b go through operators.AffineOp (rhs.flat of "
                        "pde_heat_affine), nonlinear fields are out of scope")
    op, bound = as_operator(vector_field)
    if isinstance(op, RowShardedOp):
        raise NotImplementedError("solver_rk does not take row-sharded operators (the stage kernels have no halo exchange or "
                                  "all-gather); use the operator itself")
    if isinstance(op, RbfGramOp) and op.X.requires_grad:
        raise NotImplementedError("solver_rk does not return the gradient with respect to the kernel inputs X; pass X.detach()")
    fn = _RkFn if _RK_ADJOINTS[adjoint] == "discrete" else _RkBacksolveFn

    def solve(y0, *p):
        params = (tuple(bound) if bound is not None else ()) + tuple(p)
        cparams = op.constrain(*params)
        n = op.size(*cparams) if isinstance(op, NativeOp) else y0.numel()  # a callback's state is whatever it is handed
        if isinstance(op, AffineOp):  # the scheme on (y, 1) is, stage by stage, the scheme on y' = A y + b
            Y0 = AffineOp.lift(_states_of(y0, n - 1).reshape(-1, n - 1))
            y1 = AffineOp.drop(fn.apply(op, tab, dts, Y0, *cparams))
            return y1.reshape(y0.shape), {"num_matvecs": len(dts) * tab.order, "num_applies": len(dts) * len(tab.b)}
        if y0.numel() == n:
            Y0 = y0.reshape(1, n)
        elif y0.dim() >= 2 and y0.shape[0] * n == y0.numel():  # one more dimension than the operator's state: a batch
            Y0 = y0.reshape(y0.shape[0], n)
        else:
            raise ValueError(f"a state of shape {tuple(y0.shape)} does not match the operator's {n} unknowns")
        y1 = fn.apply(op, tab, dts, Y0, *cparams)
        info = {"num_matvecs": len(dts) * tab.order, "num_applies": len(dts) * len(tab.b)}
        return y1.reshape(y0.shape), info

    return solve


def solver_rk(t0, t1, vector_field, /, *, num_steps, method, adjoint="discrete"):
    """Fixed-step explicit Runge-Kutta solve of y' = A y from t0 to t1 in ``num_steps`` equal steps (the reference's solver_diffrax,
    util/pde_util.py:196-237, on linear fields).  ``method``: a name of ``rk_tableaux``; ``adjoint``: "discrete" (also
    "recursive_checkpoint" / "direct": discretise-then-differentiate, the exact gradient of the scheme) or "backsolve" (the
    continuous adjoint).  ``vector_field``: a native operator, a bound one (``rhs.flat``) or a ``CallbackOp``.  ``solve(y0, *p)`` ->
    ``(y1, info)``; a state of any shape is flattened; a leading batch dimension is taken when y0 holds more than one state of the
    operator's size.  info["num_matvecs"] = num_steps x order is the reference's proxy, info["num_applies"] = num_steps x stages the
    true count.  t0, t1 are plain numbers (not differentiable)."""
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError("num_steps must be at least 1")
    dt = (float(t1) - float(t0)) / num_steps
    return _rk_solver((dt,) * num_steps, vector_field, method, adjoint)


solver_diffrax = solver_rk


RK_STATUS = {_lib.RK_OK: "ok", _lib.RK_MAX_ATTEMPTS: "max_attempts", _lib.RK_STEP_TOO_SMALL: "step_too_small", _lib.RK_NONFINITE: "nonfinite"}
RK_ADAPTIVE_CHUNK = 8  # attempts the driver enqueues between two reads of its control block


def _rk_adaptive_forward(op, cparams, pair, cfg, Y0, keep_ys):
    """One mfx_rk_solve_adaptive call on detached tensors -> (y1 (p, n), ys (p, n_accepted + 1, n) or None, dts, info struct)."""
    lib = _lib.get()
    Y0 = Y0.contiguous()
    p, n = Y0.shape
    dt, dev = Y0.dtype, Y0.device
    max_steps = int(cfg["max_steps"])
    call = DriverCall(op, cparams, dt, n)
    pstruct = rk_tableaux.pair_struct(pair)
    y1 = torch.empty_like(Y0)
    ys = torch.empty((p, max_steps + 1, n), dtype=dt, device=dev) if keep_ys else None
    dts = (C.c_double * max_steps)()
    info = _lib.RkAdaptiveInfo()
    ws = call.take(lambda desc: lib.mfx_rk_adaptive_workspace_bytes(desc, C.byref(pstruct), n, p, max_steps), device=dev, visible=(Y0, y1, ys))
    call.run(lib.mfx_rk_solve_adaptive, C.byref(pstruct), cfg["t0"], cfg["t1"], cfg["dt0"], cfg["rtol"], cfg["atol"], max_steps, max_steps,
             int(cfg.get("chunk", RK_ADAPTIVE_CHUNK)), _lib.ptr(Y0), n, n, p, _lib.ptr(y1), n, _lib.ptr(ys), dts, C.byref(info), 0,
             _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    if info.status != _lib.RK_OK:
        raise RuntimeError(f"{RK_STATUS.get(info.status, info.status)}: {lib.mfx_last_error().decode()}")
    steps = int(info.n_accepted)
    if ys is not None:
        ys = ys[:, : steps + 1].contiguous()  # what mfx_rk_solve would have kept for these steps
    return y1, ys, tuple(dts[:steps]), info


def _adaptive_fn(base):
    """``base`` (_RkFn or _RkBacksolveFn) with the forward replaced by the adaptive solve: the backward is ``base``'s, on the accepted
    steps as constants.  ``cfg`` (a dict) carries the controller's settings in and ``dts`` / the counters out."""

    class _Fn(base):
        @staticmethod
        def forward(ctx, op, pair, cfg, Y0, *cparams):
            tensors = stash_params(ctx, cparams)
            _lib.require_device(Y0, *tensors)
            keep = base is _RkFn and any(ctx.needs_input_grad)
            y1, ys, dts, info = _rk_adaptive_forward(op, cparams, pair, cfg, Y0, keep)
            cfg["dts"], cfg["num_rejected"] = dts, int(info.n_rejected)
            ctx.op, ctx.tab, ctx.dts = op, pair.tab, dts
            ctx.save_for_backward(ys if base is _RkFn else y1, *tensors)
            return y1

    return _Fn


_RkAdaptiveFn, _RkAdaptiveBacksolveFn = _adaptive_fn(_RkFn), _adaptive_fn(_RkBacksolveFn)


def _initial_step(apply, Y0, t0, t1, order, rtol, atol):
    """scipy's select_initial_step (Hairer, Norsett & Wanner, Solving ODEs I, II.4) per state, the smallest over the batch: two
    operator applications in torch, fp64 norms."""
    def rms(x):
        return torch.sqrt(torch.mean(x.double() ** 2, dim=-1))

    interval = t1 - t0
    scale = atol + Y0.abs().double() * rtol
    f0 = apply(Y0)
    d0, d1 = rms(Y0.double() / scale), rms(f0.double() / scale)
    h0 = torch.where((d0 < 1e-5) | (d1 < 1e-5), torch.full_like(d0, 1e-6), 0.01 * d0 / d1).clamp(max=interval)
    f1 = apply((Y0.double() + h0[:, None] * f0.double()).to(Y0.dtype))
    d2 = rms((f1.double() - f0.double()) / scale) / h0
    dmax = torch.maximum(d1, d2)
    h1 = torch.where(dmax <= 1e-15, torch.clamp(h0 * 1e-3, min=1e-6), (0.01 / dmax.clamp(min=1e-300)) ** (1.0 / order))
    return float(torch.minimum(100 * h0, h1).clamp(max=interval).min())


def solver_rk_adaptive(t0, t1, vector_field, /, *, method="dopri5", rtol, atol, dt0=None, max_steps=4096, adjoint="discrete"):
    """Adaptive-step explicit Runge-Kutta solve of y' = A y from t0 to t1 on the embedded pair ``method`` (``rk_tableaux.get_pair``:
    dopri5, bosh3, heun) with the step-size controller of scipy's ``solve_ivp``: one ``mfx_rk_solve_adaptive`` call, the step size held
    and updated on the device.  A batch shares ONE step sequence (the largest error norm over the states decides).  ``dt0``: the first
    proposal; None takes scipy's ``select_initial_step`` (two operator applications).  ``max_steps`` bounds the ATTEMPTS, rejected ones
    included, and the iterates kept for the discrete adjoint ((max_steps + 1) states while the solve runs, n_accepted + 1 afterwards).
    Operators, batches and the AffineOp lift are ``solver_rk``'s; for an AffineOp the error norm runs over the lifted state (y, 1).

    ``solve(y0, *p)`` -> ``(y1, info)``, info: ``num_steps`` (accepted), ``num_rejected``, ``num_applies`` (attempts x stages),
    ``num_matvecs`` (num_steps x order, the reference's proxy), ``dts`` (the accepted step sizes) and ``status``.  Any end other than
    reaching t1 raises ``RuntimeError`` that starts with the status: max_attempts, step_too_small, nonfinite.

    Gradients are those of the FIXED-step solve on the accepted steps: ``mfx_rk_adjoint`` on the kept iterates (adjoint="discrete") or
    ``mfx_rk_backsolve`` from y1 (adjoint="backsolve"), each with the recorded ``dts``.  The controller is NOT differentiated: the
    dependence of the step sizes on y0 and on the parameters is ignored, as in the usual discretise-then-differentiate adjoints."""
    if adjoint not in _RK_ADJOINTS:
        raise ValueError(f"adjoint must be one of {sorted(_RK_ADJOINTS)}, got {adjoint!r}")
    pair = rk_tableaux.get_pair(method)
    t0, t1, rtol, atol, max_steps = float(t0), float(t1), float(rtol), float(atol), int(max_steps)
    if not t1 > t0:
        raise ValueError(f"t1 = {t1} must be greater than t0 = {t0}")
    if max_steps < 1:
        raise ValueError("max_steps must be at least 1")
    if not isinstance(vector_field, (NativeOp, BoundOp, CallbackOp, RowShardedOp)):
        raise TypeError("solver_rk_adaptive integrates LINEAR autonomous fields y' = A y: vector_field must be a linear operator -- a native "
                        "operator, op.bind(*params) (rhs.flat of the stencil vector fields) or operators.CallbackOp(fn) -- not a "
                        f"plain callable ({type(vector_field).__name__})")
    op, bound = as_operator(vector_field)
    if isinstance(op, RowShardedOp):
        raise NotImplementedError("solver_rk_adaptive does not take row-sharded operators (the stage kernels have no halo exchange or "
                                  "all-gather, the error norm no all-reduce)")
    if isinstance(op, RbfGramOp) and op.X.requires_grad:
        raise NotImplementedError("solver_rk_adaptive does not return the gradient with respect to the kernel inputs X; pass X.detach()")
    fn = _RkAdaptiveFn if _RK_ADJOINTS[adjoint] == "discrete" else _RkAdaptiveBacksolveFn

    def solve(y0, *p, chunk=RK_ADAPTIVE_CHUNK):
        params = (tuple(bound) if bound is not None else ()) + tuple(p)
        cparams = op.constrain(*params)
        n = op.size(*cparams) if isinstance(op, NativeOp) else y0.numel()
        affine = isinstance(op, AffineOp)
        Y0 = _states_of(y0, n - 1 if affine else n).reshape(-1, n - 1 if affine else n)
        if affine:
            Y0 = AffineOp.lift(Y0)
        cfg = {"t0": t0, "t1": t1, "rtol": rtol, "atol": atol, "max_steps": max_steps, "chunk": chunk}
        if dt0 is None:
            with torch.no_grad():
                cfg["dt0"] = _initial_step(lambda Y: op(Y, *params), Y0.detach(), t0, t1, pair.order, rtol, atol)
        else:
            cfg["dt0"] = float(dt0)
        y1 = fn.apply(op, pair, cfg, Y0, *cparams)
        if affine:
            y1 = AffineOp.drop(y1)
        steps, rejected = len(cfg["dts"]), cfg["num_rejected"]
        info = {"num_steps": steps, "num_rejected": rejected, "num_applies": (steps + rejected) * len(pair.tab.b),
                "num_matvecs": steps * pair.order, "dts": cfg["dts"], "status": "ok"}
        return y1.reshape(y0.shape), info

    return solve


def solver_euler(ts, vector_field, /):
    """util/pde_util.py:177-193: explicit Euler over the (possibly non-uniform) grid ``ts``, discrete adjoint."""
    ts = [float(t) for t in (ts.tolist() if hasattr(ts, "tolist") else ts)]
    return _rk_solver([b - a for a, b in zip(ts[:-1], ts[1:])], vector_field, "euler", "discrete")


def sampler_lanczos(*, mean, cov_matvec, num, lanczos_rank):
    """util/pde_util.py:335-356: samples  mean + |eps| Q^T K^(1/2) Q eps/|eps|  from N(mean, A) via Lanczos."""

    def sample(key):
        tridiag = lanczos.tridiag(cov_matvec, lanczos_rank, reortho="full")
        if torch.is_tensor(key):
            eps = key
        else:
            gen = torch.Generator(device=mean.device)
            gen.manual_seed(int(key))
            eps = torch.randn((num, mean.numel()), dtype=mean.dtype, device=mean.device, generator=gen)
        norm = torch.linalg.vector_norm(eps, dim=-1, keepdim=True)
        u = eps / norm
        (Q, (diag, off)), _ = tridiag(u)  # Q (num, k, n)
        K = torch.diag_embed(diag) + torch.diag_embed(off, 1) + torch.diag_embed(off, -1)
        w, v = torch.linalg.eigh(K)
        w = torch.clamp_min(w, 0.0)
        factor = (v * torch.sqrt(w)[..., None, :]) @ v.transpose(-1, -2)
        coeff = torch.einsum("bkn,bn->bk", Q, u)
        return norm * torch.einsum("bkn,bk->bn", Q, torch.einsum("bkl,bl->bk", factor, coeff)) + mean.reshape(1, -1)

    return sample


def stencil_laplacian(dx):
    """util/pde_util.py:18-20."""
    return torch.tensor([[0.0, 1.0, 0.0], [1.0, -2.0, 1.0], [0.0, 1.0, 0.0]], dtype=torch.float64) / dx**2


def stencil_advection_diffusion(dx):
    """util/pde_util.py:23-28 (asymmetric: the advection part changes sign under a flip)."""
    diffusion = torch.tensor([[0.0, 1.0, 0.0], [1.0, -2.0, 1.0], [0.0, 1.0, 0.0]], dtype=torch.float64) / dx**2
    advection = torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, -1.0], [0.0, -1.0, 0.0]], dtype=torch.float64) / (2 * dx)
    return diffusion + advection


def boundary_dirichlet():
    """util/pde_util.py:146-150: zero padding by one cell.  ``pad.kind`` names the rule for the native operator."""

    def pad(x, /):
        return torch.nn.functional.pad(x, (1, 1, 1, 1))

    pad.kind = "dirichlet"
    return pad


def boundary_neumann():
    """util/pde_util.py:153-157: edge padding by one cell (the nearest cell, per axis)."""

    def pad(x, /):
        return torch.nn.functional.pad(x[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]

    pad.kind = "neumann"
    return pad


def _boundary_kind(boundary):
    kind = boundary if isinstance(boundary, str) else getattr(boundary, "kind", None)
    if kind not in ("dirichlet", "neumann"):
        raise TypeError("boundary must be boundary_dirichlet() or boundary_neumann() (the native stencil operator implements these "
                        "two padding rules; an arbitrary pad callable has no kind)")
    return kind


def _stencil_rhs(form, stencil, boundary, coef, shape, drift=None):
    """rhs(x) on (ny, nx) / (2, ny, nx) states through StencilOp; ``rhs.flat`` (when the grid is known up front): the bound
    operator on flattened states, for solver_expm / expm_arnoldi / arnoldi.hessenberg -- with a drift the bordered AffineOp on
    (state, 1)."""
    kind = _boundary_kind(boundary)
    blocks = 1 if form == "heat" else 2
    ops = {}

    def operator(grid):
        if grid not in ops:
            ops[grid] = StencilOp(grid, stencil, form=form, boundary=kind)
        return ops[grid]

    def rhs(x, /):
        if x.dim() != blocks + 1 or (blocks == 2 and x.shape[0] != 2):
            raise ValueError(f"expected a state of shape {'(ny, nx)' if blocks == 1 else '(2, ny, nx)'}, got {tuple(x.shape)}")
        op = operator(tuple(x.shape[-2:]))
        fx = (op(x.reshape(-1)) if coef is None else op(x.reshape(-1), coef.to(x.dtype))).reshape(x.shape)
        return fx if drift is None else fx + drift

    if shape is not None and drift is None:
        rhs.flat = operator(tuple(shape)).bind(*(() if coef is None else (coef,)))
    elif shape is not None:
        rhs.flat = AffineOp(operator(tuple(shape))).bind(*(() if coef is None else (coef,)), drift.reshape(-1))
    return rhs


def pde_heat(c: float, /, stencil, *, boundary, shape=None):
    """util/pde_util.py:74-87: rhs(u) = c conv(stencil, pad(u)); the constant is folded into the stencil weights.  ``shape``
    (ny, nx), optional: also provide ``rhs.flat``."""

    def parametrize():
        return _stencil_rhs("heat", c * torch.as_tensor(stencil, dtype=torch.float64), boundary, None, shape)

    return parametrize, {}


def pde_heat_affine(c: float, drift_like, /, stencil, *, boundary):
    """util/pde_util.py:90-103: pde_heat plus a drift field.  ``rhs(x)`` adds it in torch; ``rhs.flat`` is the bordered linear
    operator ``AffineOp(StencilOp(...))`` on (u, 1), bound to the drift, for solver_expm / solver_rk / solver_euler."""

    def parametrize(*, drift):
        return _stencil_rhs("heat", c * torch.as_tensor(stencil, dtype=torch.float64), boundary, None, tuple(drift_like.shape), drift=drift)

    return parametrize, {"drift": torch.empty_like(drift_like)}


def pde_heat_anisotropic(scale_like, /, stencil, *, constrain, boundary):
    """util/pde_util.py:106-123: rhs(u, du) = (-constrain(scale) o conv(stencil, pad(u)), du)."""

    def parametrize(*, scale):
        return _stencil_rhs("heat2", stencil, boundary, constrain(scale), tuple(scale_like.shape))

    return parametrize, {"scale": torch.empty_like(scale_like)}


def pde_wave_anisotropic(scale_like, /, stencil, *, constrain, boundary):
    """util/pde_util.py:126-143: rhs(u, du) = (du, constrain(scale) o conv(stencil, pad(u)))."""

    def parametrize(*, scale):
        return _stencil_rhs("wave", stencil, boundary, constrain(scale), tuple(scale_like.shape))

    return parametrize, {"scale": torch.empty_like(scale_like)}


def wave_operator(res: int, dx: float, *, boundary: str = "neumann", device=None, dtype=torch.float64):
    """The anisotropic wave right-hand side  d/dt (u, du) = (du, scale o Lap u)  (util/pde_util.py:126-143 with
    boundary_neumann :153-157 or boundary_dirichlet :146-150) as a NON-symmetric sparse operator on the flattened
    state (2 res^2,).  Returns (CsrOp, values_fn): ``values_fn(scale)`` maps the (res, res) positive coefficient field
    to the stored CSR values (differentiable), so  op(v, values_fn(scale))  is the matvec."""
    import scipy.sparse

    if boundary not in ("neumann", "dirichlet"):
        raise ValueError(boundary)
    n2 = res * res
    idx = np.arange(n2).reshape(res, res)
    ii, jj = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    st = np.array([[0.0, 1.0, 0.0], [1.0, -2.0, 1.0], [0.0, 1.0, 0.0]]) / dx**2  # stencil_laplacian (util/pde_util.py:18-20)
    r_l, c_l, w_l = [], [], []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            sw = st[di + 1, dj + 1]
            if sw == 0.0:
                continue
            ni, nj = ii + di, jj + dj
            inside = (ni >= 0) & (ni < res) & (nj >= 0) & (nj < res)
            if boundary == "neumann":  # jnp.pad(mode="edge"): the padded value is the nearest interior cell
                ni, nj, keep = np.clip(ni, 0, res - 1), np.clip(nj, 0, res - 1), np.ones_like(inside)
            else:                      # zero padding: the term drops out
                keep = inside
            r_l.append(idx[keep])
            c_l.append(idx[ni[keep], nj[keep]])
            w_l.append(np.full(int(keep.sum()), sw))
    lap = scipy.sparse.coo_matrix((np.concatenate(w_l), (np.concatenate(r_l), np.concatenate(c_l))), shape=(n2, n2)).tocsr()
    lap.sum_duplicates()
    lap = lap.tocoo()
    # state (u, du): d/dt u = du (identity block), d/dt du = scale o Lap u;  value = w * (scale[coef] if coef >= 0 else 1)
    rows = np.concatenate([np.arange(n2), n2 + lap.row])
    cols = np.concatenate([n2 + np.arange(n2), lap.col])
    w = np.concatenate([np.ones(n2), lap.data])
    coef = np.concatenate([np.full(n2, -1), lap.row])
    op, wv, order = CsrOp.from_coo(rows, cols, w, 2 * n2, device)
    wv = wv.to(dtype)
    coef_t = torch.as_tensor(np.asarray(coef)[order.numpy()], device=device)
    # CSR order: rows 0 .. n2-1 hold the identity block (one entry each), rows n2 .. 2 n2 - 1 the Laplacian block, so the
    # entries that depend on scale[r] are the contiguous range crow[n2 + r] .. crow[n2 + r + 1]
    seg = (op.crow[n2:].to(torch.int64) - n2).contiguous()
    gather = torch.clamp_min(coef_t, 0)
    is_lap = coef_t >= 0

    class _Values(torch.autograd.Function):
        """values = w * scale[row] on the Laplacian block.  The backward is a per-row segment sum via a cumulative sum
        (torch's generic gather backward sorts all 6e6 indices: 50 ms at res = 1000)."""

        @staticmethod
        def forward(ctx, s):
            return torch.where(is_lap, wv * s[gather], wv)

        @staticmethod
        def backward(ctx, g):
            gw = (g * wv)[n2:].double()
            cs = torch.cat([gw.new_zeros(1), torch.cumsum(gw, 0)])
            return (cs[seg[1:]] - cs[seg[:-1]]).to(g.dtype)

    def values_fn(scale):
        return _Values.apply(scale.reshape(-1))

    return op, values_fn
