"""Native operator objects: the explicit-parameter replacement for the reference's matvec closures.

The reference passes ``matvec(v, *params)`` callables and relies on ``jax.closure_convert`` to make
captured hyper-parameters differentiable (arnoldi.py:21-23).  Here a *native operator* is a small
object that (i) is itself callable as ``op(v, *params)`` -- so it can be handed to
``lanczos.tridiag`` / ``arnoldi.hessenberg`` / ``lanczos.integrand_spd`` wherever the reference takes
a matvec -- and (ii) knows how to describe itself to libmfx (``struct mfx_operator``) so that the
whole Krylov loop, the transposed matvec and the parameter-gradient sweep run as HIP kernels.

  DenseOp()                         params = (A,)                 tests/test_lanczos/test_tridiag_forward.py:18
  CsrOp(crow, col, n)               params = (values,)            experiments/benchmarks/.../suite_sparse/benchmark.py:64-68
  RbfGramOp(X, noise_minval=...)    params = (raw_lengthscale, raw_outputscale, raw_noise)
                                                                  util/gp_util.py:151-201,225-226,525-549
                                    (and X itself when X.requires_grad: the reference's closure conversion
                                    makes the inputs its lazy kernel closes over differentiable too)
  StencilOp(shape, stencil, ...)    params = (coef,) or ()        util/pde_util.py:74-157 (3x3 heat / wave systems, matrix-free)
  GgnMlpOp(x_train, theta, widths)  params = (alpha,)             util/bnn_util.py:263-293,477-499 (GGN of an MLP + alpha I, theta fixed)
  PreconditionedOp(op, pre, s)      params = those of ``op``      P^-1/2 A P^-1/2 for a low_rank.Preconditioner held constant
  AffineOp(op)                      params = (*those of ``op``, drift)  util/pde_util.py:90-103 (y' = A y + b as [[A, b], [0, 0]] on (y, 1))
  CallbackOp(fn)                    any Python ``fn(v, *params)`` (torch ops); per-step host control

``MlpJacobian(x, theta, widths)`` is not an operator (it is rectangular): the Jacobian of the same MLP at the points x as the pair of
linear maps ``apply`` (J V) and ``t_apply`` (J^T U), for the linearised-Laplace predictive (util/bnn_util.py:206-215, 630-683).

``op.bind(*params)`` freezes the parameters into a zero-argument-parameter matvec (what the GP code
hands to ``krylov_logdet_slq``, util/gp_util.py:555-557) while keeping them differentiable.
"""

from __future__ import annotations

import copy
import ctypes as C
import math

import torch

from . import _lib


def _check_dtype(desc, t, what):
    """The descriptor's dtype is the dtype of the VECTORS; operator data of another dtype would be misread by the kernels."""
    if _lib.dtype_code(t.dtype) != desc.dtype:
        want = "float32" if desc.dtype == _lib.MFX_F32 else "float64"
        raise TypeError(f"{what} must have the dtype of the vectors it is applied to ({want}), got {t.dtype}")


class NativeOp:
    kind = None

    # ---- differentiable map from user parameters to the tensors the kernels consume -------------
    def constrain(self, *params):
        return params

    def fill(self, desc: _lib.Operator, *cparams):
        raise NotImplementedError

    def new_grads(self, *cparams):
        """-> (OpGrads struct, tuple of zero-initialised gradient tensors aligned with cparams)."""
        raise NotImplementedError

    def descriptor(self, cparams, dtype, n):
        desc = _lib.Operator()
        desc.kind = self.kind
        desc.dtype = _lib.dtype_code(dtype)
        desc.n = n
        self.fill(desc, *cparams)
        # The descriptor borrows device pointers of the constrained parameters.  `constrain` returns fresh tensors (softplus of the raw
        # values), so a caller that writes op.descriptor(op.constrain(*params), ...) holds no other reference to them: without this one
        # the caching allocator hands their memory to the next tensor the caller creates (its output, say) and the kernels read the
        # hyper-parameters out of that tensor while they write it.
        desc._params = tuple(cparams)
        return desc

    def size(self, *cparams):
        raise NotImplementedError

    # ---- op(v, *params): plain matvec through mfx_op_apply ---------------------------------------
    def __call__(self, v, *params):
        return _ApplyFn.apply(self, False, v, *self.constrain(*params))

    def bind(self, *params):
        return BoundOp(self, params)


class BoundOp:
    """An operator with its parameters attached: ``bound(v)`` is the matvec, and the Krylov drivers
    recover ``(op, params)`` to keep the parameters differentiable (explicit closure conversion)."""

    def __init__(self, op, params):
        self.op, self.params = op, tuple(params)

    def __call__(self, v):
        return self.op(v, *self.params)


def _refuse_input_grad(op):
    if isinstance(op, RbfGramOp) and op.X.requires_grad:
        raise NotImplementedError("the gradient with respect to the kernel inputs X is not available on row-sharded operators "
                                  "(it needs the whole (n, d) gradient all-reduced and the halo of X); pass X.detach(), or shard "
                                  "the probes instead of the rows")


class RowShardedOp:
    """A native operator whose rows -- and the rows of every Krylov vector -- are sharded over the ranks of a
    ``distributed.RowComm``.  Hand it to ``lanczos.tridiag(reortho="full")`` / ``arnoldi.hessenberg`` /
    ``lanczos.integrand_spd`` in place of the operator: vectors are then this rank's row shards (p, nrows), H and the
    SLQ values come out replicated, parameter gradients complete (summed over the row group)."""

    def __init__(self, op, comm, exchange="auto"):
        if not isinstance(op, NativeOp):
            raise TypeError("row sharding needs a native operator (DenseOp, CsrOp, RbfGramOp)")
        if isinstance(op, StencilOp):
            raise NotImplementedError("row sharding a StencilOp needs a halo exchange of the grid rows next to a shard's edge, which is "
                                      "not implemented; shard the probes, or assemble the system (pde_util.wave_operator) as a CsrOp")
        if isinstance(op, PreconditionedOp):
            raise NotImplementedError("row sharding a PreconditionedOp is not implemented: L would need its rows sharded and L^T v "
                                      "all-reduced, as the row-sharded PCG does; shard the probes")
        if isinstance(op, AffineOp):
            raise NotImplementedError("row sharding an AffineOp is not implemented: the border row and column belong to no shard; "
                                      "shard the probes")
        if isinstance(op, GgnMlpOp):
            raise NotImplementedError("row sharding a GgnMlpOp is not implemented: every output row sums over all samples; shard the probes")
        _refuse_input_grad(op)
        self.op, self.comm = op, comm
        # sparse operators: neighbour exchange of the entries this rank's rows read (the halo of a stencil) instead of
        # all-gathering the whole iterate; plans for A and A^T (collective: every rank of the row group builds them here)
        self.plans = None
        if exchange == "auto":
            exchange = isinstance(op, CsrOp) and comm.world > 1
        if exchange:
            if not isinstance(op, CsrOp):
                raise TypeError("the neighbour exchange needs a sparse (CSR) operator")
            self.plans = (comm.plan_exchange(op.crow, op.col), comm.plan_exchange(op.t_crow, op.t_col))

    def bind(self, *params):
        return BoundOp(self, params)

    def constrain(self, *params):
        _refuse_input_grad(self.op)
        return self.op.constrain(*params)

    def posterior_variance(self, *args, **kwargs):
        raise NotImplementedError("the predictive variance is not available on row-sharded operators (it needs K(X, xs) and the "
                                  "solves on the whole operator); use the operator itself")

    def posterior_covariance(self, *args, **kwargs):
        raise NotImplementedError("the predictive covariance is not available on row-sharded operators (it needs K(X, xs) and the "
                                  "solves on the whole operator); use the operator itself")

    def __call__(self, v, *params):
        """this rank's rows of A v from the row shard of v (gathers v first; not differentiable -- the Krylov drivers
        use the fused device path instead)"""
        with torch.no_grad():
            cparams = self.op.constrain(*params)
            V = v if v.dim() == 2 else v[None]
            full = self.comm.gather_rows(V.contiguous())
            desc = self.op.descriptor(cparams, V.dtype, self.comm.n)
            desc.row0, desc.nrows = self.comm.row0, self.comm.nrows
            ws = _lib.workspace(desc, self.comm.n, 1, V.shape[0], V.device)
            y = torch.empty_like(V)
            _lib.check(_lib.get().mfx_op_apply(C.byref(desc), _lib.ptr(full), self.comm.n, _lib.ptr(y), self.comm.nrows,
                                               V.shape[0], 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(V.device)))
        return y if v.dim() == 2 else y[0]


class _ApplyFn(torch.autograd.Function):
    """y = A(theta) x (or A^T x); backward = A^T dy and the parameter sweep with batch = p."""

    @staticmethod
    def forward(ctx, op, transpose, v, *cparams):
        _lib.require_device(v, *cparams)
        lib = _lib.get()
        V = (v if v.dim() == 2 else v[None]).contiguous()
        p, n = V.shape
        desc = op.descriptor(cparams, V.dtype, n)
        ws = _lib.workspace(desc, n, 1, p, V.device)
        y = torch.empty_like(V)
        _lib.check(
            lib.mfx_op_apply(C.byref(desc), _lib.ptr(V), n, _lib.ptr(y), n, p, int(transpose),
                             _lib.ptr(ws), ws.numel(), _lib.stream_ptr(V.device))
        )
        ctx.op, ctx.transpose, ctx.vdim = op, transpose, v.dim()
        ctx.save_for_backward(V, *cparams)
        return y if v.dim() == 2 else y[0]

    @staticmethod
    def backward(ctx, dy):
        V, *cparams = ctx.saved_tensors
        op, lib = ctx.op, _lib.get()
        DY = (dy if dy.dim() == 2 else dy[None]).contiguous()
        p, n = V.shape
        desc = op.descriptor(cparams, V.dtype, n)
        ws = _lib.workspace(desc, n, 1, p, V.device)
        dv = torch.empty_like(V)
        _lib.check(
            lib.mfx_op_apply(C.byref(desc), _lib.ptr(DY), n, _lib.ptr(dv), n, p, int(not ctx.transpose),
                             _lib.ptr(ws), ws.numel(), _lib.stream_ptr(V.device))
        )
        gstruct, grads = op.new_grads(*cparams)
        L, R = (DY, V) if not ctx.transpose else (V, DY)
        _lib.check(
            lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), n, _lib.ptr(R), n, p, C.byref(gstruct),
                                  _lib.ptr(ws), ws.numel(), _lib.stream_ptr(V.device))
        )
        return (None, None, dv if ctx.vdim == 2 else dv[0], *grads)


class _CrossApplyFn(torch.autograd.Function):
    """y = K(xnew, X) v; backward = K(X, xnew) dy (mfx_gram_cross_apply_t) and one mfx_gram_cross_vjp call for the lengthscale,
    outputscale, xnew and X gradients -- each computed only when asked for."""

    @staticmethod
    def forward(ctx, op, xnew, v, *cparams):
        _lib.require_device(xnew, v, *cparams)
        V = (v if v.dim() == 2 else v[None]).contiguous()
        xnew = xnew.contiguous()
        if xnew.dim() != 2 or xnew.shape[1] != op.d or V.shape[1] != op.n:
            raise ValueError(f"cross_apply: xnew {tuple(xnew.shape)}, v {tuple(v.shape)} do not match X {tuple(op.X.shape)}")
        m, p = xnew.shape[0], V.shape[0]
        desc = op.descriptor(cparams, V.dtype, op.n)
        lib = _lib.get()
        ws = _lib.scratch(int(lib.mfx_gram_cross_workspace_bytes(C.byref(desc), m)), V.device)
        y = torch.empty((p, m), dtype=V.dtype, device=V.device)
        _lib.check(lib.mfx_gram_cross_apply(C.byref(desc), _lib.ptr(xnew), m, _lib.ptr(V), op.n, _lib.ptr(y), m, p,
                                            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(V.device)))
        ctx.op, ctx.vdim = op, v.dim()
        ctx.save_for_backward(xnew, V, *cparams)
        return y if v.dim() == 2 else y[0]

    @staticmethod
    def backward(ctx, dy):
        xnew, V, *cparams = ctx.saved_tensors
        op, lib = ctx.op, _lib.get()
        need = ctx.needs_input_grad  # (op, xnew, v, lengthscale, outputscale, noise[, X])
        DY = (dy if dy.dim() == 2 else dy[None]).contiguous()
        (p, n), m = V.shape, xnew.shape[0]
        desc = op.descriptor(cparams, V.dtype, n)
        stream = _lib.stream_ptr(V.device)
        dv = gxnew = gls = gs = gx = None
        if need[2]:
            ws = _lib.scratch(int(lib.mfx_gram_cross_workspace_bytes(C.byref(desc), m)), V.device)
            dv = torch.empty_like(V)
            _lib.check(lib.mfx_gram_cross_apply_t(C.byref(desc), _lib.ptr(xnew), m, _lib.ptr(DY), m, _lib.ptr(dv), n, p,
                                                  _lib.ptr(ws), ws.numel(), stream))
            dv = dv if ctx.vdim == 2 else dv[0]
        want_x = len(need) > 6 and need[6]
        if need[1] or need[3] or need[4] or want_x:
            st = _lib.OpGrads()
            if need[3]:
                gls = torch.zeros_like(cparams[0])
                st.lengthscale = gls.data_ptr()
            if need[4]:
                gs = torch.zeros_like(cparams[1])
                st.outputscale = gs.data_ptr()
            if want_x:
                gx = torch.zeros_like(cparams[3], memory_format=torch.contiguous_format)
                st.x = gx.data_ptr()
            if need[1]:
                gxnew = torch.zeros_like(xnew)
            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_workspace_bytes(C.byref(desc), m, p)), V.device)
            _lib.check(lib.mfx_gram_cross_vjp(C.byref(desc), _lib.ptr(xnew), m, _lib.ptr(DY), m, _lib.ptr(V), n, p, C.byref(st),
                                              _lib.ptr(gxnew), _lib.ptr(ws), ws.numel(), stream))
        return (None, gxnew, dv, gls, gs, None, *((gx,) if len(cparams) > 3 else ()))


def _kappa0(kind, dtype):
    """k(x, x) / s: the kernel's own value at distance 0, with the reference's eps inside the square roots (util/gp_util.py:69-148)."""
    if kind == "rbf":
        return 1.0
    r = math.sqrt(torch.finfo(dtype).eps)
    if kind == "matern52":
        return (1.0 + r + r * r / 3.0) * math.exp(-r)
    return (1.0 + r) * math.exp(-r) if kind == "matern32" else math.exp(-r)


def _cat_info(parts):
    """per-chunk solve info dicts -> one dict, the per-right-hand-side tensors concatenated in test-point order"""
    out = {}
    for key in parts[0]:
        vals = [p[key] for p in parts]
        out[key] = torch.cat(vals) if all(torch.is_tensor(v) and v.dim() > 0 for v in vals) else vals
    return out


class _PosteriorVarFn(torch.autograd.Function):
    """var_a = s kappa(0) - b_a^T A^-1 b_a with b_a = K(X, xs_a), A = K + noise I.  Forward: per chunk of test points, B = K(xs_c, X)
    (mfx_gram_cross_apply_t against the identity), W = solve(A, B) without grad, q = rowwise <B, W>.  Backward, with W kept from the
    forward (d var_a = d(s kappa(0)) - 2 w_a^T db_a + w_a^T dA w_a: no adjoint solve): mfx_gram_cross_vjp_dense with S = -2 vbar W
    and mfx_op_vjp_params with L = vbar W, R = W -- each only for the gradients asked for."""

    @staticmethod
    def forward(ctx, op, bound, solve, chunk, info, xs, *cparams):
        _lib.require_device(xs, *cparams)
        xs = xs.contiguous()
        (m, _), n, dt, dev = xs.shape, op.n, xs.dtype, xs.device
        desc = op.descriptor(cparams, dt, n)
        lib, stream = _lib.get(), _lib.stream_ptr(dev)
        keep = any(ctx.needs_input_grad[5:])
        W = torch.empty((m, n), dtype=dt, device=dev) if keep else None
        q = torch.empty((m,), dtype=dt, device=dev)
        parts = []
        for a0 in range(0, m, chunk):
            c = min(chunk, m - a0)
            eye = torch.eye(c, dtype=dt, device=dev)
            B = torch.empty((c, n), dtype=dt, device=dev)
            ws = _lib.scratch(int(lib.mfx_gram_cross_workspace_bytes(C.byref(desc), c)), dev)
            _lib.check(lib.mfx_gram_cross_apply_t(C.byref(desc), _lib.ptr(xs[a0 : a0 + c]), c, _lib.ptr(eye), c, _lib.ptr(B), n, c,
                                                  _lib.ptr(ws), ws.numel(), stream))
            Wc, sinfo = solve(bound, B)
            q[a0 : a0 + c] = (B * Wc).sum(-1)
            if keep:
                W[a0 : a0 + c] = Wc
            parts.append(sinfo)
        info["solve"] = _cat_info(parts)
        ctx.op, ctx.kappa0 = op, _kappa0(op.kernel, dt)
        ctx.save_for_backward(xs, W, *cparams)
        return cparams[1] * ctx.kappa0 - q

    @staticmethod
    def backward(ctx, vbar):
        xs, W, *cparams = ctx.saved_tensors
        op, lib = ctx.op, _lib.get()
        need = ctx.needs_input_grad  # (op, bound, solve, chunk, info, xs, lengthscale, outputscale, noise[, X])
        want_x = len(need) > 9 and need[9]
        (m, n), dev = W.shape, W.device
        desc = op.descriptor(cparams, W.dtype, n)
        stream = _lib.stream_ptr(dev)
        vbar = vbar.contiguous()
        gxs = gls = gs = gn = gx = None
        if need[6]:
            gls = torch.zeros_like(cparams[0])
        if need[7]:
            gs = torch.zeros_like(cparams[1])
        if need[8]:
            gn = torch.zeros_like(cparams[2])
        if want_x:
            gx = torch.zeros_like(cparams[3], memory_format=torch.contiguous_format)
        S = None
        if need[5] or need[6] or need[7] or want_x:  # -2 w_a^T db_a: the cross sweep with the dense weights S = -2 vbar W
            gxs = torch.zeros_like(xs) if need[5] else None
            S = W * (-2.0 * vbar)[:, None]
            st = _lib.OpGrads()
            st.lengthscale, st.outputscale, st.x = (None if t is None else t.data_ptr() for t in (gls, gs, gx))
            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(C.byref(desc), m)), dev)
            _lib.check(lib.mfx_gram_cross_vjp_dense(C.byref(desc), _lib.ptr(xs), m, _lib.ptr(S), n, C.byref(st), _lib.ptr(gxs),
                                                    _lib.ptr(ws), ws.numel(), stream))
        if need[6] or need[7] or need[8] or want_x:  # w_a^T dA w_a: the Gram parameter sweep with L = vbar W, R = W, batch m
            L = S.mul_(-0.5) if S is not None else W * vbar[:, None]  # (scaling by -2, then -1/2, is exact: L == vbar W bitwise)
            st = _lib.OpGrads()
            st.lengthscale, st.outputscale, st.noise, st.x = (None if t is None else t.data_ptr() for t in (gls, gs, gn, gx))
            ws = _lib.workspace(desc, n, 1, m, dev)
            _lib.check(lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), n, _lib.ptr(W), n, m, C.byref(st), _lib.ptr(ws), ws.numel(),
                                             stream))
        if gs is not None:
            gs += ctx.kappa0 * vbar.sum()
        return (None, None, None, None, None, gxs, gls, gs, gn, *((gx,) if len(cparams) > 3 else ()))


def _gram_block(op, cparams, xa, xb, out=None):
    """K(xa, xb) (ma, mb) through mfx_gram_block, outside autograd; xb None: the symmetric block K(xa, xa).  ``out``: a contiguous
    (ma, mb) tensor to fill (a row slice of a larger matrix)."""
    lib, dev = _lib.get(), xa.device
    ma, mb = xa.shape[0], (xa if xb is None else xb).shape[0]
    desc = op.descriptor(cparams, xa.dtype, op.n)
    if out is None:
        out = torch.empty((ma, mb), dtype=xa.dtype, device=dev)
    ws = _lib.scratch(int(lib.mfx_gram_block_workspace_bytes(C.byref(desc), ma, mb)), dev)
    _lib.check(lib.mfx_gram_block(C.byref(desc), _lib.ptr(xa), ma, _lib.ptr(xb), mb, _lib.ptr(out), mb, _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr(dev)))
    return out


def _gram_block_vjp(op, cparams, xa, pts, S, gxa, gpts, gls, gs):
    """accumulates the gradients of sum_ab S_ab k(xa_a, pts_b) into the tensors that are not None: mfx_gram_cross_vjp_dense on a
    descriptor whose x / n are pts / len(pts) (xa takes the X_new slot).  S (ma, len(pts)) contiguous."""
    lib, dev = _lib.get(), xa.device
    ma, mb = S.shape
    desc = op.descriptor(cparams, xa.dtype, mb)
    desc.x, desc.n = pts.data_ptr(), mb
    st = _lib.OpGrads()
    st.lengthscale, st.outputscale, st.x = (None if t is None else t.data_ptr() for t in (gls, gs, gpts))
    ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(C.byref(desc), ma)), dev)
    _lib.check(lib.mfx_gram_cross_vjp_dense(C.byref(desc), _lib.ptr(xa), ma, _lib.ptr(S), mb, C.byref(st), _lib.ptr(gxa),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))


def _symmetric_block_vjp(op, cparams, xa, S, gxa, gls, gs):
    """the same for the symmetric block K(xa, xa): both slots of every off-diagonal pair; the diagonal is the constant s kappa(0) of
    the forward (distance exactly 0), so it reaches the outputscale only"""
    off = S.clone()
    off.diagonal().zero_()
    gpts = torch.zeros_like(gxa) if gxa is not None else None
    _gram_block_vjp(op, cparams, xa, xa, off, gxa, gpts, gls, gs)
    if gxa is not None:
        gxa += gpts
    if gs is not None:
        gs += _kappa0(op.kernel, xa.dtype) * S.diagonal().sum()


class _GramBlockFn(torch.autograd.Function):
    """K(xa, xb) (mfx_gram_block; xb None: K(xa, xa)); backward = one mfx_gram_cross_vjp_dense call with the cotangent as the dense
    weights, on a descriptor over xb -- each gradient computed only when asked for."""

    @staticmethod
    def forward(ctx, op, xa, xb, *cparams):
        _lib.require_device(xa, xb, *cparams)
        xa = xa.contiguous()
        xb = None if xb is None else xb.contiguous()
        out = _gram_block(op, cparams, xa, xb)
        ctx.op, ctx.symmetric = op, xb is None
        ctx.save_for_backward(xa, *(() if xb is None else (xb,)), *cparams)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        xa, xb, cparams = (saved[0], None, saved[1:]) if ctx.symmetric else (saved[0], saved[1], saved[2:])
        need = ctx.needs_input_grad  # (op, xa, xb, lengthscale, outputscale, noise[, X])
        gxa = gxb = gls = gs = None
        if need[1] or need[2] or need[3] or need[4]:
            S = dy.contiguous()
            gxa = torch.zeros_like(xa) if need[1] else None
            gls = torch.zeros_like(cparams[0]) if need[3] else None
            gs = torch.zeros_like(cparams[1]) if need[4] else None
            if ctx.symmetric:
                _symmetric_block_vjp(ctx.op, cparams, xa, S, gxa, gls, gs)
            else:
                gxb = torch.zeros_like(xb) if need[2] else None
                _gram_block_vjp(ctx.op, cparams, xa, xb, S, gxa, gxb, gls, gs)
        return (None, gxa, gxb, gls, gs, None, *((None,) if len(cparams) > 3 else ()))


class _PosteriorCovFn(torch.autograd.Function):
    """Sigma = K(xs, xs) - B A^-1 B^T with B = K(xs, X), A = K + noise I.  Forward: per chunk of test points B_c = mfx_gram_block(xs_c, X)
    and W_c = solve(A, B_c) without grad; then Kss = the symmetric block of xs and Sigma = Kss - (B W^T + W B^T) / 2 (two torch
    products; the symmetrised form is bitwise symmetric whatever the solver left in W).
    Backward, with W = B A^-1 kept from the forward and C = (Sbar + Sbar^T) / 2 (Sigma is symmetric in its arguments, so only the
    symmetric part of the cotangent acts):
      d Sigma = dKss - dB W^T - W dB^T + W dA W^T
      <Sbar, dKss>       = <C, dKss>           the dense sweep with the weights C on the operator over xs (both slots)
      -<Sbar, dB W^T + W dB^T> = <-2 C W, dB>  mfx_gram_cross_vjp_dense with S = -2 C W
      <Sbar, W dA W^T>   = sum_a (C W)_a^T dA w_a   mfx_op_vjp_params with L = C W, R = W, batch m
    -- no adjoint solve, and each sweep only for the gradients asked for."""

    @staticmethod
    def forward(ctx, op, bound, solve, chunk, info, xs, *cparams):
        _lib.require_device(xs, *cparams)
        xs = xs.contiguous()
        (m, _), n, dt, dev = xs.shape, op.n, xs.dtype, xs.device
        X = op.X.detach()
        B = torch.empty((m, n), dtype=dt, device=dev)
        W = torch.empty((m, n), dtype=dt, device=dev)
        parts = []
        for a0 in range(0, m, chunk):
            c = min(chunk, m - a0)
            _gram_block(op, cparams, xs[a0 : a0 + c], X, out=B[a0 : a0 + c])
            W[a0 : a0 + c], sinfo = solve(bound, B[a0 : a0 + c])
            parts.append(sinfo)
        info["solve"] = _cat_info(parts)
        P = B @ W.T
        cov = _gram_block(op, cparams, xs, None) - 0.5 * (P + P.T)
        ctx.op = op
        ctx.save_for_backward(xs, W, *cparams)
        return cov

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, sbar):
        xs, W, *cparams = ctx.saved_tensors
        op, lib = ctx.op, _lib.get()
        need = ctx.needs_input_grad  # (op, bound, solve, chunk, info, xs, lengthscale, outputscale, noise[, X])
        want_x = len(need) > 9 and need[9]
        (m, n), dev = W.shape, W.device
        gxs = torch.zeros_like(xs) if need[5] else None
        gls = torch.zeros_like(cparams[0]) if need[6] else None
        gs = torch.zeros_like(cparams[1]) if need[7] else None
        gn = torch.zeros_like(cparams[2]) if need[8] else None
        gx = torch.zeros_like(cparams[3], memory_format=torch.contiguous_format) if want_x else None
        if not (need[5] or need[6] or need[7] or need[8] or want_x):
            return (None,) * (6 + len(cparams))
        Cs = 0.5 * (sbar + sbar.T)
        CW = Cs @ W
        if need[5] or need[6] or need[7]:  # <C, dKss>
            _symmetric_block_vjp(op, cparams, xs, Cs, gxs, gls, gs)
        if need[5] or need[6] or need[7] or want_x:  # <-2 C W, dB>
            _gram_block_vjp(op, cparams, xs, op.X.detach(), CW * -2.0, gxs, gx, gls, gs)
        if need[6] or need[7] or need[8] or want_x:  # sum_a (C W)_a^T dA w_a
            desc = op.descriptor(cparams, W.dtype, n)
            st = _lib.OpGrads()
            st.lengthscale, st.outputscale, st.noise, st.x = (None if t is None else t.data_ptr() for t in (gls, gs, gn, gx))
            ws = _lib.workspace(desc, n, 1, m, dev)
            _lib.check(lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(CW), n, _lib.ptr(W), n, m, C.byref(st), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr(dev)))
        return (None, None, None, None, None, gxs, gls, gs, gn, *((gx,) if len(cparams) > 3 else ()))


class DenseOp(NativeOp):
    """matvec(v, A) = A @ v."""

    kind = _lib.OP_DENSE

    def constrain(self, A):
        return (A.contiguous(),)

    def size(self, A):
        return A.shape[0]

    def fill(self, desc, A):
        _check_dtype(desc, A, "DenseOp: the matrix")
        if A.dim() != 2 or A.shape[0] != A.shape[1]:
            raise ValueError(f"DenseOp expects a square matrix, got {tuple(A.shape)}")
        desc.dense_a = A.data_ptr()
        desc.lda = A.stride(0)

    def new_grads(self, A):
        g = torch.zeros_like(A)
        s = _lib.OpGrads()
        s.dense_a = g.data_ptr()
        return s, (g,)


class CsrOp(NativeOp):
    """matvec(v, vals) = CSR(vals; crow, col) @ v; differentiable w.r.t. all stored values."""

    kind = _lib.OP_CSR

    def __init__(self, crow, col, n, device=None):
        device = device if device is not None else crow.device
        self.n = int(n)
        self.crow = crow.to(device=device, dtype=torch.int32).contiguous()
        self.col = col.to(device=device, dtype=torch.int32).contiguous()
        counts = (self.crow[1:] - self.crow[:-1]).to(torch.int64)
        self.row = torch.repeat_interleave(torch.arange(self.n, device=device, dtype=torch.int32), counts)
        self.nnz = int(self.col.numel())
        # CSR structure of A^T (for the Arnoldi adjoint's A^T lambda): stable sort of entries by column
        key = self.col.to(torch.int64) * self.n + self.row.to(torch.int64)
        perm = torch.argsort(key, stable=True)
        self.t_perm = perm.to(torch.int32).contiguous()
        self.t_col = self.row[perm].contiguous()
        tcounts = torch.bincount(self.col.to(torch.int64), minlength=self.n)
        self.t_crow = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), torch.cumsum(tcounts, 0)]).to(torch.int32)
        # longest row of A and of A^T (one host read at construction): decides fused-step vs 8-lanes-per-row kernels in libmfx
        self.max_row_nnz = int(max(int(counts.max()) if self.nnz else 0, int(tcounts.max()) if self.nnz else 0))

    @classmethod
    def from_coo(cls, row, col, vals, n, device):
        """COO (e.g. scipy.io.mmread's symmetric expansion, util/exp_util.py:35-42) -> (op, values)."""
        row = torch.as_tensor(row, dtype=torch.int64)
        col = torch.as_tensor(col, dtype=torch.int64)
        order = torch.argsort(row * n + col, stable=True)
        row, col = row[order], col[order]
        crow = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(row, minlength=n), 0)])
        op = cls(crow.to(device), col.to(device), n, device=device)
        return op, torch.as_tensor(vals)[order].to(device), order

    def constrain(self, vals):
        return (vals.contiguous(),)

    def size(self, vals):
        return self.n

    def fill(self, desc, vals):
        _check_dtype(desc, vals, "CsrOp: the stored values")
        if vals.numel() != self.nnz:
            raise ValueError(f"CsrOp expects {self.nnz} values, got {vals.numel()}")
        desc.crow, desc.col, desc.row = self.crow.data_ptr(), self.col.data_ptr(), self.row.data_ptr()
        desc.val, desc.nnz, desc.max_row_nnz = vals.data_ptr(), self.nnz, self.max_row_nnz
        desc.t_crow, desc.t_col, desc.t_perm = self.t_crow.data_ptr(), self.t_col.data_ptr(), self.t_perm.data_ptr()

    def new_grads(self, vals):
        g = torch.zeros_like(vals)
        s = _lib.OpGrads()
        s.val = g.data_ptr()
        return s, (g,)


class StencilOp(NativeOp):
    """The reference's PDE vector fields (util/pde_util.py:74-157) without a matrix: a padded 3x3 convolution S of the (ny, nx) grid
    ``u``, scaled by a coefficient field.  On flattened states (row-major grid, blocks stacked):

      form="heat"   v = u        (ny nx,)    ->  coef o S u              pde_heat
      form="heat2"  v = (u, du)  (2 ny nx,)  ->  (-coef o S u, du)       pde_heat_anisotropic
      form="wave"   v = (u, du)  (2 ny nx,)  ->  (du, coef o S u)        pde_wave_anisotropic

    ``stencil`` is 3x3 in the reference's orientation, ``convolve2d(stencil, padded, "valid")``; boundary="dirichlet" pads with
    zeros, "neumann" with the nearest cell.  ``op(v, coef)`` takes the field as (ny, nx) or flat and is differentiable with respect
    to both; ``op(v)`` is the operator without a field (all ones).  The apply, the transposed apply and the field gradient are
    HIP kernels (csrc/mfx_stencil.hip); nothing is assembled."""

    kind = _lib.OP_STENCIL
    _FORMS = {"heat": _lib.STENCIL_HEAT, "heat2": _lib.STENCIL_HEAT2, "wave": _lib.STENCIL_WAVE}
    _BOUNDARIES = {"dirichlet": _lib.BOUNDARY_DIRICHLET, "neumann": _lib.BOUNDARY_NEUMANN}

    def __init__(self, shape, stencil, *, form="wave", boundary="neumann"):
        if form not in self._FORMS:
            raise ValueError(f"form must be one of {sorted(self._FORMS)}")
        if boundary not in self._BOUNDARIES:
            raise ValueError(f"boundary must be one of {sorted(self._BOUNDARIES)}")
        self.ny, self.nx = (int(shape), int(shape)) if isinstance(shape, int) else (int(shape[0]), int(shape[1]))
        if self.ny < 1 or self.nx < 1:
            raise ValueError(f"StencilOp: the grid must be at least 1 x 1, got {self.ny} x {self.nx}")
        w = torch.as_tensor(stencil).detach().to(device="cpu", dtype=torch.float64)
        if tuple(w.shape) != (3, 3):
            raise ValueError(f"StencilOp expects a 3 x 3 stencil, got {tuple(w.shape)}")
        # convolve2d flips the stencil: weights[(dr + 1) * 3 + (dc + 1)] multiplies u_pad[r + dr, c + dc]
        self.weights = [float(x) for x in torch.flip(w, (0, 1)).reshape(-1)]
        self.form, self.boundary = form, boundary
        self.cells = self.ny * self.nx
        self.n = self.cells if form == "heat" else 2 * self.cells

    def constrain(self, coef=None):
        return () if coef is None else (coef.reshape(-1).contiguous(),)

    def size(self, *_):
        return self.n

    def fill(self, desc, coef=None):
        if coef is not None:
            _check_dtype(desc, coef, "StencilOp: the coefficient field")
            if coef.numel() != self.cells:
                raise ValueError(f"StencilOp expects a field of {self.ny} x {self.nx} = {self.cells} values, got {coef.numel()}")
            desc.val = coef.data_ptr()
        desc.st_ny, desc.st_nx = self.ny, self.nx
        desc.st_form, desc.st_boundary = self._FORMS[self.form], self._BOUNDARIES[self.boundary]
        desc.st_w = (C.c_double * 9)(*self.weights)

    def new_grads(self, coef=None):
        s = _lib.OpGrads()
        if coef is None:
            return s, ()
        g = torch.zeros_like(coef)
        s.val = g.data_ptr()
        return s, (g,)


_MLP_FIXED = ("holds theta and {x} fixed: a gradient with respect to them needs third derivatives of the network, which the reference "
              "never takes; pass detached tensors")


def _mlp_problem(who, x, theta, widths, activation, xname):
    """The checks GgnMlpOp and MlpJacobian share -> (widths, number of parameters, x as (N, d_in))."""
    if activation not in ("tanh", "relu"):
        raise ValueError("activation must be 'tanh' or 'relu'")
    if theta.requires_grad or x.requires_grad:
        raise NotImplementedError(f"{who} " + _MLP_FIXED.format(x=xname))
    widths = tuple(int(w) for w in widths)
    nl = len(widths) - 1
    if not 1 <= nl <= _lib.GGN_MAX_LAYERS or min(widths) < 1:
        raise ValueError(f"{who}: widths {widths} must name 1..{_lib.GGN_MAX_LAYERS} layers of at least one unit")
    n = sum((wi + 1) * wo for wi, wo in zip(widths[:-1], widths[1:]))
    if theta.dim() != 1 or theta.numel() != n:
        raise ValueError(f"{who}: widths {widths} have {n} parameters, theta has shape {tuple(theta.shape)}")
    x2 = x.reshape(x.shape[0], -1)
    if x2.shape[0] < 1 or x2.shape[1] != widths[0] or x2.dtype != theta.dtype or x2.device != theta.device:
        raise ValueError(f"{who}: {xname} {tuple(x.shape)} ({x2.dtype}, {x2.device}) does not match widths[0] = "
                         f"{widths[0]} and theta ({theta.dtype}, {theta.device})")
    return widths, n, x2


def _mlp_tape(theta, x, widths, activation, softmax):
    """{"act": [a_0 = x, ..., a_{L-1}], "dact": [None, phi'(z_1), ..., phi'(z_{L-1})], "logits", "prob" (None without softmax)}"""
    with torch.no_grad():
        a, off = x.contiguous(), 0
        act, dact = [a], [None]
        nl = len(widths) - 1
        for l in range(1, nl + 1):
            wi, wo = widths[l - 1], widths[l]
            z = a @ theta[off + wo : off + wo + wi * wo].reshape(wi, wo) + theta[off : off + wo]
            off += (wi + 1) * wo
            if l < nl:
                if activation == "tanh":
                    a = torch.tanh(z)
                    d = 1 - a * a
                else:
                    a = torch.relu(z)
                    d = (z > 0).to(z.dtype)
                act.append(a.contiguous())
                dact.append(d.contiguous())
        prob = torch.softmax(z, dim=-1).contiguous() if softmax else None
    return {"act": act, "dact": dact, "logits": z, "prob": prob}


def _mlp_net(widths, theta, tape, loss_code):
    """struct mfx_ggn_net over a tape (a host struct of device pointers: it must not outlive the tensors)"""
    nl = len(widths) - 1
    net = _lib.GgnNet()
    net.nlayers, net.loss, net.nsamples = nl, loss_code, tape["act"][0].shape[0]
    net.width = (C.c_int32 * (_lib.GGN_MAX_LAYERS + 1))(*widths)
    net.theta = theta.data_ptr()
    for l in range(nl):
        net.act[l] = tape["act"][l].data_ptr()
        if l >= 1:
            net.dact[l] = tape["dact"][l].data_ptr()
    if tape["prob"] is not None:
        net.prob = tape["prob"].data_ptr()
    return net


class GgnMlpOp(NativeOp):
    """The generalised Gauss-Newton matrix of an MLP plus a shift, matrix-free (the reference's ggn_vp_parallel inside
    callibration_loss, util/bnn_util.py:263-293, 477-499):

      A(alpha) v = sum_i J_i^T H_i J_i v + alpha v,   J_i = d f(theta; x_i) / d theta,   H_i = loss Hessian in the logits

    ``theta`` is the flat parameter vector in the order of flax's ravel_pytree for ``model_mlp``: per layer the bias (width[l]), then
    the kernel (width[l-1], width[l]) row-major; ``widths = (d_in, ..., c)``.  theta and x_train are FIXED (the calibration loss is
    differentiated in alpha alone): everything that depends on them -- layer inputs, activation slopes, softmax probabilities -- is
    computed once here with torch ops and kept as ``op.tape``; one application is one fused HIP pass over that tape
    (csrc/mfx_ggn.hip).  ``op(v, alpha)`` is differentiable in v and alpha; gradients with respect to theta or x_train would need
    third derivatives and are refused."""

    kind = _lib.OP_GGN
    _LOSSES = {"cross_entropy": _lib.GGN_CROSS_ENTROPY, "mse": _lib.GGN_MSE}

    def __init__(self, x_train, theta, widths, *, activation="tanh", loss="cross_entropy"):
        if loss not in self._LOSSES:
            raise ValueError(f"loss must be one of {sorted(self._LOSSES)}")
        self.widths, self.n, x = _mlp_problem("GgnMlpOp", x_train, theta, widths, activation, "x_train")
        self.activation, self.loss = activation, loss
        self.theta = theta.detach().contiguous()
        self.tape = self._build_tape(x)
        self.net = _mlp_net(self.widths, self.theta, self.tape, self._LOSSES[loss])  # the descriptor's ctx points here

    def _build_tape(self, x):
        """{"act": [a_0 = x, ..., a_{L-1}], "dact": [None, phi'(z_1), ..., phi'(z_{L-1})], "logits", "prob" (None for mse)}"""
        return _mlp_tape(self.theta, x, self.widths, self.activation, self.loss == "cross_entropy")

    def jacobian(self):
        """The network Jacobian at the operator's own samples, over its own tape: the tensors are shared, nothing is recomputed."""
        return MlpJacobian._over(self.widths, self.activation, self.theta, self.tape)

    def diagonal(self, alpha=None):
        """The exact diagonal sum_i diag(J_i^T H_i J_i) over the operator's own tape, (P,), in one fused HIP pass (mfx_ggn_diag: c
        backward sweeps per sample, squared where they are produced; the reference's exact_diagonal takes N c^2 gradients).  Entrywise
        >= 0.  ``alpha`` (a tensor or a number) is added with a torch add, so the result is differentiable in it; the diagonal
        itself is a constant."""
        _lib.require_device(self.theta)
        lib, code, dev = _lib.get(), _lib.dtype_code(self.theta.dtype), self.theta.device
        need = int(lib.mfx_ggn_diag_workspace_bytes(C.byref(self.net), code))
        if need < 0:  # the query refuses what the call would: the call names the reason and the code
            _lib.check(lib.mfx_ggn_diag(C.byref(self.net), code, None, None, 0, None))
        ws = _lib.scratch(need, dev)
        diag = torch.empty(self.n, dtype=self.theta.dtype, device=dev)
        with _lib.busy(ws):
            _lib.check(lib.mfx_ggn_diag(C.byref(self.net), code, _lib.ptr(diag), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return diag if alpha is None else diag + alpha

    def constrain(self, alpha):
        return (alpha.reshape(1),)

    def size(self, *_):
        return self.n

    def fill(self, desc, alpha):
        _check_dtype(desc, self.theta, "GgnMlpOp: theta and the tape")
        _check_dtype(desc, alpha, "GgnMlpOp: alpha")
        if alpha.numel() != 1 or alpha.device != self.theta.device:
            raise ValueError("GgnMlpOp: alpha is one value on the device of theta")
        desc.noise = alpha.data_ptr()
        desc.ctx = C.addressof(self.net)

    def new_grads(self, alpha):
        g = torch.zeros_like(alpha)
        s = _lib.OpGrads()
        s.noise = g.data_ptr()
        return s, (g,)


class MlpJacobian:
    """The Jacobian J = d f(theta; x_i) / d theta of the MLP of ``GgnMlpOp`` at the points x, (N c) x P, as a pair of linear maps over a
    tape built once (include/mfx.h, next to struct mfx_ggn_net; csrc/mfx_ggn.hip):

      jac.apply(V)     J V:    (p, P) -> (p, N, c),  (P,) -> (N, c)        mfx_mlp_jac_apply
      jac.t_apply(U)   J^T U:  (p, N, c) -> (p, P),  (N, c) -> (P,)        mfx_mlp_jac_t_apply

    ``jac.logits`` (N, c) is the mean prediction f(theta; x), ``jac.n_params`` = P.  theta and x are FIXED, as for GgnMlpOp; both maps
    are differentiable in their argument (they are linear: the backward of one is the other).  ``jac.rows(i0, i1)`` is the Jacobian
    at the points i0 .. i1 - 1 over row slices of the same tape."""

    def __init__(self, x, theta, widths, *, activation="tanh"):
        widths, _, x2 = _mlp_problem("MlpJacobian", x, theta, widths, activation, "x")
        theta = theta.detach().contiguous()
        self._set(widths, activation, theta, _mlp_tape(theta, x2, widths, activation, False))

    def _set(self, widths, activation, theta, tape):
        self.widths, self.activation, self.theta, self.tape = widths, activation, theta, tape
        self.n_params = sum((wi + 1) * wo for wi, wo in zip(widths[:-1], widths[1:]))
        self.n_samples, self.n_out = tape["act"][0].shape[0], widths[-1]
        self.logits = tape["logits"]
        self.net = _mlp_net(widths, theta, {**tape, "prob": None}, 0)  # the maps read neither the loss nor the softmax

    @classmethod
    def _over(cls, widths, activation, theta, tape):
        new = cls.__new__(cls)
        new._set(widths, activation, theta, tape)
        return new

    def rows(self, i0, i1):
        """The Jacobian at the points i0 .. i1 - 1: row slices of the tape tensors (views), nothing rebuilt."""
        if not 0 <= i0 < i1 <= self.n_samples:
            raise ValueError(f"MlpJacobian.rows: [{i0}, {i1}) is not a range of the {self.n_samples} points")
        cut = lambda t: None if t is None else t[i0:i1]  # noqa: E731  (rows of a contiguous matrix: contiguous)
        tape = {"act": [cut(t) for t in self.tape["act"]], "dact": [cut(t) for t in self.tape["dact"]],
                "logits": cut(self.tape["logits"]), "prob": cut(self.tape["prob"])}
        return MlpJacobian._over(self.widths, self.activation, self.theta, tape)

    def apply(self, V):
        return _JacFn.apply(self, False, V)

    def t_apply(self, U):
        return _JacFn.apply(self, True, U)

    # ---- the two calls, outside autograd ----
    def _check(self, what, t):
        _lib.require_device(t, self.theta)
        if t.dtype != self.theta.dtype:
            raise TypeError(f"MlpJacobian: {what} must have the dtype of theta and the tape ({self.theta.dtype}), got {t.dtype}")
        if t.device != self.theta.device:
            raise ValueError(f"MlpJacobian: {what} is on {t.device}, theta and the tape on {self.theta.device}")

    def _forward(self, V):
        self._check("V", V)
        batched = V.dim() == 2
        V2 = (V if batched else V[None]).contiguous()
        if V2.dim() != 2 or V2.shape[1] != self.n_params or V2.shape[0] < 1:
            raise ValueError(f"MlpJacobian.apply: V {tuple(V.shape)} must be (p, {self.n_params}) or ({self.n_params},)")
        p = V2.shape[0]
        out = torch.empty((p, self.n_samples, self.n_out), dtype=V2.dtype, device=V2.device)
        with torch.cuda.device(V2.device):
            _lib.check(_lib.get().mfx_mlp_jac_apply(C.byref(self.net), _lib.dtype_code(V2.dtype), _lib.ptr(V2), self.n_params, p,
                                                    _lib.ptr(out), _lib.stream_ptr(V2.device)))
        return out if batched else out[0]

    def _transpose(self, U):
        self._check("U", U)
        batched = U.dim() == 3
        U3 = (U if batched else U[None]).contiguous()
        if U3.dim() != 3 or tuple(U3.shape[1:]) != (self.n_samples, self.n_out) or U3.shape[0] < 1:
            raise ValueError(f"MlpJacobian.t_apply: U {tuple(U.shape)} must be (p, {self.n_samples}, {self.n_out}) or "
                             f"({self.n_samples}, {self.n_out})")
        p, lib, code = U3.shape[0], _lib.get(), _lib.dtype_code(U3.dtype)
        need = int(lib.mfx_mlp_jac_workspace_bytes(C.byref(self.net), code, p))
        if need < 0:  # the query refuses what the call would: the call names the reason and the code
            _lib.check(lib.mfx_mlp_jac_t_apply(C.byref(self.net), code, _lib.ptr(U3), p, None, self.n_params, None, 0, None))
        ws = _lib.scratch(need, U3.device)
        Y = torch.empty((p, self.n_params), dtype=U3.dtype, device=U3.device)
        with _lib.busy(ws):
            _lib.check(lib.mfx_mlp_jac_t_apply(C.byref(self.net), code, _lib.ptr(U3), p, _lib.ptr(Y), self.n_params, _lib.ptr(ws),
                                               ws.numel(), _lib.stream_ptr(U3.device)))
        return Y if batched else Y[0]


class _JacFn(torch.autograd.Function):
    """J V (transpose False) or J^T U (True); both are linear in their argument, so the backward of one is the other."""

    @staticmethod
    def forward(ctx, jac, transpose, t):
        ctx.jac, ctx.transpose = jac, transpose
        return jac._transpose(t) if transpose else jac._forward(t)

    @staticmethod
    def backward(ctx, dy):
        return None, None, _JacFn.apply(ctx.jac, not ctx.transpose, dy)


def softplus(x, beta=1.0, threshold=20.0):
    """torch-style thresholded softplus, as util/gp_util.py:187-201 mirrors it."""
    return torch.nn.functional.softplus(x, beta=beta, threshold=threshold)


class RbfGramOp(NativeOp):
    """(K(X, X) + noise I) v with the reference's scaled-kernel parametrisation, matrix-free.

    kernel: "rbf" (kernel_scaled_rbf, util/gp_util.py:151-184), "matern32" (:69-107), "matern12" (:110-148),
    "matern52" ((1 + r + r^2 / 3) exp(-r), r = sqrt(5 s + eps); kernel_scaled_matern_52 -- not in the reference).

    params = (raw_lengthscale [() or (d,)], raw_outputscale (), raw_noise ());
    lengthscale = softplus(raw_l), outputscale = softplus(raw_s)         (util/gp_util.py:164-165)
    noise = noise_minval + softplus(raw_noise)                            (util/gp_util.py:187-201,222)

    precision: arithmetic of the fp32 Gram kernels for wide probe batches --
      "f16x3" (default)  matvec AND parameter-gradient GEMM emulated on the f16 matrix pipe (hi/lo split,
                         3 products, fp32 accumulate): 2.1x faster end to end, accuracy on par with "fp32";
      "f16x3-matvec"     split matvec, exact fp32 gradient GEMM: the most accurate mode against fp64;
      "fp32"             exact fp32 MFMA everywhere.
    fp64 operators ignore it.

    X may require grad (deep-kernel inputs ``net(features)``, learned warpings): ``constrain`` then returns X as a fourth
    tensor, so every autograd Function of the package returns its gradient (libmfx's input sweep, ``mfx_op_grads.x``)
    and it reaches the caller's tensor through ``X.contiguous()``.  Not on row-sharded operators.
    """

    kind = _lib.OP_RBF
    _MODES = {"fp32": _lib.RBF_FP32, "f16x3-matvec": _lib.RBF_F16X3_MATVEC, "f16x3": _lib.RBF_F16X3}

    _KERNELS = {"rbf": _lib.KERNEL_RBF, "matern12": _lib.KERNEL_MATERN12, "matern32": _lib.KERNEL_MATERN32,
                "matern52": _lib.KERNEL_MATERN52}

    def __init__(self, X, noise_minval=0.0, precision="f16x3", kernel="rbf"):
        if X.dim() != 2:
            raise ValueError("RbfGramOp expects inputs of shape (n, d)")
        if precision not in self._MODES:
            raise ValueError(f"precision must be one of {sorted(self._MODES)}")
        if kernel not in self._KERNELS:
            raise ValueError(f"kernel must be one of {sorted(self._KERNELS)}")
        self.kernel = kernel
        self.X = X.contiguous()
        self.n, self.d = X.shape
        self.noise_minval = noise_minval
        self.precision = precision

    def constrain(self, raw_lengthscale, raw_outputscale, raw_noise):
        dt = self.X.dtype
        ls = softplus(raw_lengthscale).to(dt).reshape(-1)
        if ls.numel() not in (1, self.d):
            raise ValueError(f"raw_lengthscale must have shape () or ({self.d},)")
        s = softplus(raw_outputscale).to(dt).reshape(1)
        nz = (self.noise_minval + softplus(raw_noise)).to(dt).reshape(1)
        if self.X.requires_grad:
            return (ls.contiguous(), s, nz, self.X)
        return (ls.contiguous(), s, nz)

    def size(self, *_):
        return self.n

    def fill(self, desc, ls, s, nz, X=None):
        if self.X.dtype != ls.dtype:
            raise TypeError("RbfGramOp: X and the hyper-parameters must share a dtype")
        _check_dtype(desc, self.X, "RbfGramOp: the inputs X")
        desc.x, desc.d = self.X.data_ptr(), self.d
        desc.ard = int(ls.numel() == self.d)
        desc.rbf_mode = self._MODES[self.precision]
        desc.kernel_fn = self._KERNELS[self.kernel]
        desc.lengthscale, desc.outputscale, desc.noise = ls.data_ptr(), s.data_ptr(), nz.data_ptr()

    def cross_apply(self, xnew, v, *params):
        """K(xnew, X) v (no noise term): the prior cross-covariance matvec of the posterior mean
        (util/gp_util.py:299-305).  xnew (m, d), v (n,) or (p, n) -> (m,) or (p, m).  Differentiable with respect to xnew,
        v, the lengthscale and outputscale parameters and X (when X.requires_grad); the noise gets no gradient here."""
        cparams = self.constrain(*params)
        return _CrossApplyFn.apply(self, xnew.to(self.X.dtype), v, *cparams)

    def posterior_variance(self, xs, solve, *params, chunk=64, return_info=False):
        """The latent predictive variance s kappa(0) - diag(K(xs, X) A^-1 K(X, xs)), A = K(X, X) + noise I, at the test points xs
        (m, d) -> (m,), where kappa(0) is the kernel's value at distance 0 (1 for RBF; the Matern forms keep the reference's eps).
        Not clamped: rounding can make a value slightly negative.

        solve(A, B) -> (W, info) is any solver of cg.* (a pcg.* solver with its preconditioner bound in a lambda); it runs without
        grad on batches of at most ``chunk`` right-hand sides B = K(xs_c, X) (c, n).  Differentiable with respect to xs, the three
        parameters and X (when X.requires_grad) without another solve: the backward reuses the solutions W.  When a gradient is
        required W is kept from the forward to the backward: m * n elements of X's dtype (1024 test points against 131 072
        training points in fp32: 512 MiB), plus as much again during the backward.  return_info=True returns (variance, info) with
        info["solve"] the solver's info per right-hand side, in test-point order."""
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"posterior_variance: chunk must be >= 1, got {chunk}")
        if xs.dim() != 2 or xs.shape[1] != self.d or xs.shape[0] < 1:
            raise ValueError(f"posterior_variance: xs {tuple(xs.shape)} must be (m >= 1, {self.d})")
        cparams = self.constrain(*params)
        info = {}
        var = _PosteriorVarFn.apply(self, self.bind(*params), solve, chunk, info, xs.to(self.X.dtype), *cparams)
        return (var, info) if return_info else var

    def _check_points(self, what, x):
        if x.dim() != 2 or x.shape[1] != self.d or x.shape[0] < 1:
            raise ValueError(f"{what} {tuple(x.shape)} must be (m >= 1, {self.d})")

    def gram_block(self, xa, xb, *params):
        """The dense block K(xa, xb) of the prior kernel matrix, (ma, mb), written by mfx_gram_block: no noise term, the Gram
        operator's conventions (inputs over the lengthscale, distance clamped at 0, eps inside Matern's square root).  xb=None:
        the symmetric block K(xa, xa), bitwise symmetric, its diagonal s kappa(0) exactly.  Uses the operator's kernel, dtype and d
        only -- not its X: pass ``op.X`` as xb for K(xa, X) (the gradient then reaches X through that argument).  Differentiable
        with respect to xa, xb, the lengthscale and outputscale parameters; the noise gets no gradient."""
        self._check_points("gram_block: xa", xa)
        if xb is not None:
            self._check_points("gram_block: xb", xb)
            xb = xb.to(self.X.dtype)
        cparams = self.constrain(*params)
        return _GramBlockFn.apply(self, xa.to(self.X.dtype), xb, *cparams)

    def posterior_covariance(self, xs, solve, *params, chunk=64, return_info=False):
        """The joint latent predictive covariance K(xs, xs) - K(xs, X) A^-1 K(X, xs), A = K(X, X) + noise I, of the test points xs
        (m, d) -> (m, m), bitwise symmetric; its diagonal is posterior_variance.  Not clamped or jittered: rounding can leave it
        slightly indefinite (gp_util.posterior_samples takes a jitter).

        solve(A, B) -> (W, info) as in posterior_variance, without grad on batches of at most ``chunk`` right-hand sides
        B = K(xs_c, X), which mfx_gram_block writes directly.  Differentiable with respect to xs, the three parameters and X (when
        X.requires_grad) without another solve.  Memory: B and W are (m, n) each and the result (m, m), in X's dtype; W is kept
        for the backward, which holds one more (m, n) product (1024 test points against 131 072 training points in fp32: 512 MiB
        each).  return_info=True returns (covariance, info) with info["solve"] as posterior_variance lays it out."""
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"posterior_covariance: chunk must be >= 1, got {chunk}")
        self._check_points("posterior_covariance: xs", xs)
        cparams = self.constrain(*params)
        info = {}
        cov = _PosteriorCovFn.apply(self, self.bind(*params), solve, chunk, info, xs.to(self.X.dtype), *cparams)
        return (cov, info) if return_info else cov

    def new_grads(self, ls, s, nz, X=None):
        g = (torch.zeros_like(ls), torch.zeros_like(s), torch.zeros_like(nz))
        st = _lib.OpGrads()
        st.lengthscale, st.outputscale, st.noise = (t.data_ptr() for t in g)
        if X is not None:  # X carried as a constrained tensor: the input sweep writes dG/dX (n, d)
            gx = torch.zeros_like(X, memory_format=torch.contiguous_format)
            st.x = gx.data_ptr()
            g = (*g, gx)
        return st, g


def _rows(t):
    """(tensor, leading dimension) of a 2-d tensor as libmfx reads it: rows of unit stride, any row pitch >= the row length."""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


class _RffFn(torch.autograd.Function):
    """(S, n) = RandomFeatures.evaluate; backward = one mfx_rff_grad_x call onto x."""

    @staticmethod
    def forward(ctx, feats, x, ls, s):
        x, ldx = _rows(x)
        out = torch.empty((feats.num_samples, x.shape[0]), dtype=x.dtype, device=x.device)
        _lib.check(_lib.get().mfx_rff_apply(*feats._args(x, ldx, ls, s), _lib.ptr(out), out.shape[1], _lib.stream_ptr(x.device)))
        ctx.feats = feats
        ctx.save_for_backward(x, ls, s)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, ls, s = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        g, ldg = _rows(dy)
        dx = torch.empty((x.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
        _lib.check(_lib.get().mfx_rff_grad_x(*ctx.feats._args(x, x.stride(0) if x.shape[0] > 1 else x.shape[1], ls, s), _lib.ptr(g), ldg,
                                             _lib.ptr(dx), dx.shape[1], _lib.stream_ptr(x.device)))
        return None, dx, None, None


class RandomFeatures:
    """S prior sample paths f_s(x) = c sum_j cos(omega_j . x / l + b_j) W_sj, c = sqrt(2 outputscale / m), of a stationary GP prior:
    a random-Fourier-feature expansion whose frequencies follow the kernel's spectral density (the prior term of Matheron's
    rule, gp_util.likelihood_condition_pathwise).  Frequencies omega (m, d) in units of 1 / lengthscale, phases b (m) and weights
    W (S, m) are drawn ONCE, from a torch generator seeded from ``key`` as hutchinson.sampler_normal seeds its own (the same key gives
    the same paths; they are drawn in fp64 on the device of ``like`` and cast to its dtype):

        rbf                              omega ~ N(0, I)
        matern12 / matern32 / matern52   omega = z sqrt(2 nu / g), z ~ N(0, I_d), g a sum of 2 nu = 1 / 3 / 5 squared standard
                                         normals per feature (the multivariate-t spectral density of the MFX_KERNEL_* formulas)
        b ~ U[0, 2 pi),  W ~ N(0, 1)

    Explicit tensors ``omega=``, ``phase=``, ``weights=`` are taken as given instead (then the key is not used for them).

    ``evaluate(x, lengthscale, outputscale)`` -> (S, n) for points x (n, d): mfx_rff_apply, the (n, m) feature matrix never stored.
    lengthscale (() or (d,)) and outputscale arrive constrained, as RbfGramOp.constrain returns them.  Differentiable with respect to
    x ONLY (backward: one mfx_rff_grad_x call).  Gradients with respect to the lengthscale, the outputscale, W, omega or b are
    REFUSED: a tensor among them that requires grad raises ValueError.  CPU tensors raise; there is no fallback.

    A finite m under-represents the prior variance far from the data: the sample variance of the paths is outputscale only in
    expectation over the frequencies, with a relative spread of order 1 / sqrt(m)."""

    _NU2 = {"rbf": None, "matern12": 1, "matern32": 3, "matern52": 5}

    def __init__(self, key, *, kernel, dim, num_features, num_samples, like, omega=None, phase=None, weights=None):
        if kernel not in self._NU2:
            raise ValueError(f"kernel must be one of {sorted(self._NU2)}")
        self.kernel, self.dim, self.num_features, self.num_samples = kernel, int(dim), int(num_features), int(num_samples)
        if self.dim < 1 or self.dim > 1024:
            raise ValueError(f"RandomFeatures: dim must be in 1..1024, got {dim}")
        if self.num_features < 1 or self.num_samples < 1:
            raise ValueError(f"RandomFeatures: num_features and num_samples must be >= 1, got {num_features} and {num_samples}")
        _lib.dtype_code(like.dtype)
        dtype, device = like.dtype, like.device
        m, d, S = self.num_features, self.dim, self.num_samples
        gen = None
        if omega is None or phase is None or weights is None:
            if key is None or torch.is_tensor(key):
                missing = [name for name, t in (("omega", omega), ("phase", phase), ("weights", weights)) if t is None]
                raise ValueError(f"RandomFeatures: {', '.join(missing)} must be drawn, which needs an integer key (or (seed, offset)), "
                                 f"got {'a tensor' if torch.is_tensor(key) else None}; or pass them explicitly")
            seed = key[0] ^ (key[1] * 0x9E3779B1) if isinstance(key, tuple) else key
            gen = torch.Generator(device=device)
            gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)

        def normal(*shape):
            return torch.randn(shape, dtype=torch.float64, device=device, generator=gen)

        # the draws are consumed in a fixed order (z, g, b, W) whichever of them are given explicitly
        if omega is None:
            omega = normal(m, d)
            nu2 = self._NU2[kernel]
            if nu2 is not None:
                omega = omega * torch.sqrt(nu2 / normal(m, nu2).square().sum(dim=1, keepdim=True))
        if phase is None:
            phase = 2 * math.pi * torch.rand((m,), dtype=torch.float64, device=device, generator=gen)
        if weights is None:
            weights = normal(S, m)
        for name, t, shape in (("omega", omega, (m, d)), ("phase", phase, (m,)), ("weights", weights, (S, m))):
            if tuple(t.shape) != shape:
                raise ValueError(f"RandomFeatures: {name} {tuple(t.shape)} must be {shape}")
            if t.device != device:
                raise ValueError(f"RandomFeatures: {name} is on {t.device}, `like` on {device}")
        self.omega, self.phase, self.weights = omega.to(dtype), phase.to(dtype), weights.to(dtype)
        # what the kernel reads: frequencies and phases in revolutions (divided in fp64, then rounded once)
        self._omega_rev = (self.omega.double() / (2 * math.pi)).to(dtype).contiguous()
        self._phase_rev = (self.phase.double() / (2 * math.pi)).to(dtype).contiguous()
        self._weights, self._ldw = _rows(self.weights.detach())  # rows of unit stride, made once and kept: the kernels read this tensor

    def _args(self, x, ldx, ls, s):
        W, ldw = self._weights, self._ldw
        return (_lib.dtype_code(x.dtype), _lib.ptr(x), ldx, x.shape[0], self.dim, _lib.ptr(self._omega_rev), _lib.ptr(self._phase_rev),
                self.num_features, _lib.ptr(ls), int(ls.numel() == self.dim), _lib.ptr(s),
                _lib.ptr(W), ldw, self.num_samples)

    def evaluate(self, x, lengthscale, outputscale):
        """The S paths at the points x (n, d) -> (S, n); see the class docstring for what is differentiable and what is refused."""
        for name, t in (("lengthscale", lengthscale), ("outputscale", outputscale), ("weights", self.weights), ("omega", self.omega),
                        ("phase", self.phase)):
            if t.requires_grad:
                raise ValueError(f"RandomFeatures.evaluate: the gradient with respect to {name} is refused (only x is differentiable "
                                 "through the random features); pass it detached")
        _lib.require_device(x, lengthscale, outputscale, self.weights)
        for name, t in (("x", x), ("lengthscale", lengthscale), ("outputscale", outputscale)):
            if t.device != self.weights.device:
                raise ValueError(f"RandomFeatures.evaluate: {name} is on {t.device}, the features on {self.weights.device}")
        if x.dim() != 2 or x.shape[1] != self.dim or x.shape[0] < 1:
            raise ValueError(f"RandomFeatures.evaluate: x {tuple(x.shape)} must be (n >= 1, {self.dim})")
        dtype = self.weights.dtype
        if x.dtype != dtype:
            raise TypeError(f"RandomFeatures.evaluate: x must have the dtype of the features ({dtype}), got {x.dtype}")
        ls = lengthscale.to(dtype).reshape(-1).contiguous()
        if ls.numel() not in (1, self.dim):
            raise ValueError(f"RandomFeatures.evaluate: lengthscale must have shape () or ({self.dim},)")
        s = outputscale.to(dtype).reshape(-1)
        if s.numel() != 1:
            raise ValueError("RandomFeatures.evaluate: outputscale must be a scalar")
        return _RffFn.apply(self, x, ls, s)


class PreconditionedOp(NativeOp):
    """B(theta) = S A(theta) S with S = P^-1/2 for a ``low_rank.Preconditioner`` P = s I + L L^T that is held CONSTANT:
    log det A = log det P + tr log B, and the gradient of the right-hand side with respect to theta is that of log det A, so SLQ
    with adjoints on B plus ``logdet()`` is the estimator of the same quantity with a spectrum clustered at 1.

    ``op`` is any native operator, ``pre`` the preconditioner, ``s`` its shift (detached here: no gradient flows through P).
    Parameters, ``constrain``, ``size`` and the gradient fields are those of ``op`` (X of a kernel-Gram operator included); the two
    applications of S per matvec run in libmfx (``MFX_OP_PRECOND``, csrc/mfx_lowrank.hip)."""

    kind = _lib.OP_PRECOND

    def __init__(self, op, pre, s):
        if not isinstance(op, NativeOp) or isinstance(op, PreconditionedOp):
            raise TypeError("PreconditionedOp needs a native operator (DenseOp, CsrOp, RbfGramOp, StencilOp, GgnMlpOp) that is not "
                            "itself preconditioned")
        if isinstance(op, AffineOp):
            raise TypeError("PreconditionedOp does not take an AffineOp: the bordered matrix [[A, b], [0, 0]] is not symmetric, and "
                            "the drift gradient belongs to the affine operator alone")
        self.op, self.pre = op, pre
        self.s = s.detach() if torch.is_tensor(s) else s
        self._factor = None

    def constrain(self, *params):
        return self.op.constrain(*params)

    def size(self, *cparams):
        return self.op.size(*cparams)

    def new_grads(self, *cparams):
        return self.op.new_grads(*cparams)

    def logdet(self):
        """log det P (fp64 scalar): what ``tr log B`` lacks of ``log det A``."""
        return self.pre.logdet(self.s)

    def descriptor(self, cparams, dtype, n):
        inner = self.op.descriptor(cparams, dtype, n)
        if self.pre.n != n or self.pre.lt.dtype != dtype:
            raise ValueError(f"PreconditionedOp: a preconditioner of size {self.pre.n} ({self.pre.lt.dtype}) around an operator of "
                             f"size {n} ({dtype})")
        _lib.require_device(self.pre.lt)
        if self._factor is None:
            self._factor = self.pre.inv_sqrt(self.s)
        mid, scale = self._factor
        desc = _lib.Operator()
        desc.kind, desc.dtype, desc.n = self.kind, _lib.dtype_code(dtype), n
        pc = _lib.Precond()
        pc.pc_inner = C.addressof(inner)
        pc.pc_lt, pc.pc_mid, pc.pc_scale = self.pre.lt.data_ptr(), mid.data_ptr(), scale.data_ptr()
        pc.pc_rank = self.pre.rank
        desc.ctx = C.addressof(pc)
        desc._keep = (pc, inner, mid, scale)  # the host struct and the inner descriptor live as long as the outer one
        return desc


class AffineOp(NativeOp):
    """The affine vector field y' = A(theta) y + b as a LINEAR operator on the state (y, 1), one entry longer:

      B (y, s) = (A y + s b, 0)          exp(t B) (y0, 1) = (e^{tA} y0 + t phi_1(tA) b, 1)

    so ``arnoldi.hessenberg``, ``expm_arnoldi``, ``solver_expm`` and ``solver_rk`` with both adjoints integrate the affine field through
    the drivers of linear ones (every explicit Runge-Kutta scheme on B is, stage by stage, the same scheme on y' = A y + b).  ``op`` is
    a ``DenseOp``, ``CsrOp``, ``StencilOp``, ``RbfGramOp`` or ``GgnMlpOp``; the parameters are ``(*params of op, drift)``, the drift
    with ``op``'s number of unknowns in any shape, all differentiable; ``size`` is ``op``'s plus one.  ``lift`` / ``drop`` move between
    y and (y, 1).  The border runs in libmfx (``MFX_OP_AFFINE``, csrc/mfx_affine.hip) behind the inner operator's own kernels."""

    kind = _lib.OP_AFFINE

    def __init__(self, op):
        if not isinstance(op, NativeOp) or isinstance(op, (PreconditionedOp, AffineOp)):
            raise TypeError("AffineOp needs a native operator (DenseOp, CsrOp, StencilOp, RbfGramOp, GgnMlpOp) that is neither "
                            "preconditioned nor affine itself")
        self.op = op
        self._refuse_inputs()

    def _refuse_inputs(self):
        if differentiable_inputs(self.op):
            raise NotImplementedError("AffineOp does not return the gradient with respect to the kernel inputs X of its inner "
                                      "RbfGramOp; pass X.detach()")

    @staticmethod
    def lift(y):
        """(..., n) -> (..., n + 1): a 1 appended to the last axis."""
        return torch.cat([y, y.new_ones((*y.shape[:-1], 1))], dim=-1)

    @staticmethod
    def drop(z):
        """(..., n + 1) -> (..., n): the last entry removed."""
        return z[..., :-1]

    def constrain(self, *params):
        self._refuse_inputs()
        if not params:
            raise TypeError("AffineOp: the drift is the last parameter")
        return (*self.op.constrain(*params[:-1]), params[-1].reshape(-1).contiguous())

    def size(self, *cparams):
        return self.op.size(*cparams[:-1]) + 1

    def new_grads(self, *cparams):
        s, grads = self.op.new_grads(*cparams[:-1])
        g = torch.zeros_like(cparams[-1])
        s.drift = g.data_ptr()
        return s, (*grads, g)

    def descriptor(self, cparams, dtype, n):
        drift = cparams[-1]
        inner = self.op.descriptor(cparams[:-1], dtype, n - 1)
        desc = _lib.Operator()
        desc.kind, desc.dtype, desc.n = self.kind, _lib.dtype_code(dtype), n
        _check_dtype(desc, drift, "AffineOp: the drift")
        if drift.numel() != n - 1:
            raise ValueError(f"AffineOp: a drift of {drift.numel()} values around an operator of {n - 1} unknowns")
        _lib.require_device(drift)
        af = _lib.Affine()
        af.af_inner, af.af_b = C.addressof(inner), drift.data_ptr()
        desc.ctx = C.addressof(af)
        desc._keep = (af, inner)  # the host struct and the inner descriptor live as long as the outer one
        desc._params = tuple(cparams)
        return desc


class _PtrRegistry:
    """Maps raw device pointers handed to a callback back to torch views (no copies)."""

    def __init__(self):
        self.bufs = []

    def add(self, t):
        if t is not None:
            if not t.is_contiguous():
                raise ValueError("registered buffers must be contiguous")
            self.bufs.append((t.data_ptr(), t.numel() * t.element_size(), t.view(-1)))

    def add_bytes(self, t_u8, dtype):
        es = torch.empty((), dtype=dtype).element_size()
        usable = (t_u8.numel() // es) * es
        self.bufs.append((t_u8.data_ptr(), usable, t_u8[:usable].view(dtype)))

    def view(self, ptr, ld, p, n):
        for base, nbytes, flat in self.bufs:
            if base <= ptr < base + nbytes:
                off = (ptr - base) // flat.element_size()
                return flat[off:].as_strided((p, n), (ld, 1))
        raise RuntimeError("libmfx callback received an unknown pointer")


class CallbackOp:
    """Generic Python matvec ``fn(v, *params)`` (torch ops on device tensors).

    libmfx still drives the k-loop and runs every Krylov vector kernel; only the matvec (and, in the
    adjoint, its VJP through torch.autograd -- the analogue of jax.vjp at arnoldi.py:207-208 /
    lanczos.py:328-329) is delegated.  ``fn`` acts on ONE vector; probes are looped.
    """

    kind = _lib.OP_CALLBACK

    def __init__(self, fn):
        self.fn = fn

    def constrain(self, *params):
        return params

    def __call__(self, v, *params):
        return self.fn(v, *params)

    def bind(self, *params):
        return BoundOp(self, params)

    def make(self, params, dtype, n, registry, want_grads):
        """-> (descriptor, keepalive, grad accumulators or None)."""
        params = tuple(params)
        accum = [torch.zeros_like(q) if (want_grads and torch.is_tensor(q) and q.is_floating_point()) else None for q in params]
        fn = self.fn
        failure = []

        def trampoline(_ctx, mode, xp, ldx, auxp, ldaux, yp, ldy, p, nn, _stream):
            try:
                X = registry.view(xp, ldx, p, nn)
                Y = registry.view(yp, ldy, p, nn)
                if mode == 0:
                    with torch.no_grad():
                        for b in range(p):
                            Y[b].copy_(fn(X[b], *params))
                    return 0
                AUX = registry.view(auxp, ldaux, p, nn)
                for b in range(p):
                    with torch.enable_grad():
                        live = [q.detach().requires_grad_(True) if a is not None else q for q, a in zip(params, accum)]
                        diff = [q for q, a in zip(live, accum) if a is not None]
                        if mode == 1:  # y = A^T x ; d/dtheta x^T A(theta) aux      (arnoldi.py:207-209)
                            u = AUX[b].detach().clone().requires_grad_(True)
                            out = fn(u, *live)
                            grads = torch.autograd.grad(out, [u, *diff], X[b], allow_unused=True)
                            Y[b].copy_(grads[0])
                            pg = grads[1:]
                        else:  # y = A x ; d/dtheta aux^T A(theta) x                   (lanczos.py:328-329)
                            out = fn(X[b].detach(), *live)
                            Y[b].copy_(out.detach())
                            pg = torch.autograd.grad(out, diff, AUX[b], allow_unused=True) if diff else ()
                    it = iter(pg)
                    for a in accum:
                        if a is not None:
                            g = next(it)
                            if g is not None:
                                a.add_(g)
                return 0
            except Exception as exc:  # never let an exception cross the C boundary
                failure.append(exc)
                return 1

        cb = _lib.CALLBACK_T(trampoline)
        desc = _lib.Operator()
        desc.kind = _lib.OP_CALLBACK
        desc.dtype = _lib.dtype_code(dtype)
        desc.n = n
        desc.callback = cb
        return desc, (cb, failure), accum


class DriverCall:
    """One libmfx driver call on behalf of an autograd Function, for a native, callback or row-sharded operator:

        call = DriverCall(op, cparams, dtype, n, want_grads)   # .desc; .gptr, .grads aligned with cparams; .comm (or None)
        ws = call.take(lib.mfx_..._workspace_bytes, *dims, device=dev, visible=(tensors the call hands out pointers into))
        call.run(lib.mfx_x_sharded if call.comm else lib.mfx_x, <the arguments after the descriptor and the comm>)

    It holds the two rules that are easy to get wrong: every tensor a callback may be handed is registered, and a Python exception
    captured inside the call wins over the return code."""

    def __init__(self, op, cparams, dtype, n, want_grads=False):
        self.dtype, self.reg, self.comm, self.plans, self.failure = dtype, None, None, None, ()
        self.gptr, self.grads = None, ()
        if isinstance(op, RowShardedOp):  # vectors are row shards; the descriptor is the whole operator's (n = comm.n)
            op, self.comm, self.plans = op.op, op.comm, op.plans
        if isinstance(op, CallbackOp):  # the trampoline accumulates the parameter gradients itself: no mfx_op_grads
            self.reg = _PtrRegistry()
            self.desc, (self._cb, self.failure), self.grads = op.make(cparams, dtype, n, self.reg, want_grads)
        else:
            self.desc = op.descriptor(cparams, dtype, n)
            if want_grads:
                self._gstruct, self.grads = op.new_grads(*cparams)
                self.gptr = C.byref(self._gstruct)

    def take(self, query, *dims, device, visible=()):
        """The workspace of the call, ``query(desc[, comm], *dims)`` bytes from ``_lib._take``, taken ONCE; ``visible``: the tensors a
        callback operator or the exchange of a row-sharded one may receive pointers into, besides the workspace itself."""
        lead = [C.byref(self.desc)] + ([C.byref(self.comm.size_query())] if self.comm is not None else [])
        self.ws = ws = _lib.scratch(int(query(*lead, *dims)), device)
        if self.reg is not None:
            for t in visible:
                self.reg.add(t)
            self.reg.add_bytes(ws, self.dtype)
        if self.comm is not None:
            self._cm, self._keep = self.comm.struct(ws, tensors=visible, plans=self.plans)
            lead[1], self.failure = C.byref(self._cm), self._keep[2]
        self.lead = lead
        return ws

    def run(self, entry, *args):
        """``entry(desc[, comm], *args)`` with the workspace marked busy for the call and nothing else; then the Python exception the
        callback trampoline or a collective captured, as the original object, in preference to the status; then the status."""
        with _lib.busy(self.ws):
            rc = entry(*self.lead, *args)
        if self.failure:
            raise self.failure[0]
        _lib.check(rc)


def reduce_grads_(comm, grads):
    """Row-sharded backward: partial sums over this rank's rows -> the complete gradients, in place, by ONE small all-reduce."""
    if comm.world > 1 and grads:
        flat = torch.cat([g.reshape(-1) for g in grads])
        comm.all_reduce_(flat)
        off = 0
        for g in grads:
            g.copy_(flat[off : off + g.numel()].reshape(g.shape))
            off += g.numel()


_TENSOR = object()  # the place of a tensor in ctx.nontensor (None is a parameter value like any other)


def stash_params(ctx, cparams):
    """Forward: the non-tensor parameters stay on ``ctx``; -> the tensors among them, for ``ctx.save_for_backward``."""
    ctx.nontensor = [_TENSOR if torch.is_tensor(q) else q for q in cparams]
    return [q for q in cparams if torch.is_tensor(q)]


def rebuild_params(ctx, tensors):
    """Backward: the parameter tuple of ``stash_params`` again, around the saved tensors."""
    it = iter(tensors)
    return tuple(next(it) if q is _TENSOR else q for q in ctx.nontensor)


KernelGramOp = RbfGramOp  # the operator covers the reference's three stationary kernels


def differentiable_inputs(op):
    """Tensors an operator closes over that need a gradient: RbfGramOp's X when it requires grad, else ()."""
    if isinstance(op, PreconditionedOp):
        return differentiable_inputs(op.op)
    return (op.X,) if isinstance(op, RbfGramOp) and op.X.requires_grad else ()


def with_inputs(op, inputs):
    """A shallow copy of ``op`` that closes over ``inputs`` (ordered as differentiable_inputs returns them) instead."""
    if not inputs:
        return op
    new = copy.copy(op)
    if isinstance(op, PreconditionedOp):
        new.op = with_inputs(op.op, inputs)
        return new
    (new.X,) = inputs
    return new


def as_operator(matvec):
    """matvec argument of the reference API -> (operator, bound-params or None)."""
    if isinstance(matvec, BoundOp):
        return matvec.op, matvec.params
    if isinstance(matvec, (NativeOp, CallbackOp, RowShardedOp)):
        return matvec, None
    if callable(matvec):
        return CallbackOp(matvec), None
    raise TypeError(f"matvec must be callable or a native operator, got {type(matvec)}")
