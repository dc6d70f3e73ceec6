"""Low-rank approximations: partial (pivoted) Cholesky and the preconditioner built from it -- MI355X build.

Same functional surface as the reference's ``matfree_extensions/low_rank.py``:

    cholesky_partial(rank=...)(lazy_kernel, n)        -> (chol (n, rank), {})
    cholesky_partial_pivot(rank=...)(lazy_kernel, n)  -> (chol (n, rank), {"success": bool})
    preconditioner(cholesky)(lazy_kernel, nrows)      -> (solve, info),   solve(v, s) = (s I + L L^T)^{-1} v

executed by libmfx (``mfx_partial_cholesky`` / ``mfx_precond_apply``).  Difference: the reference's ``lazy_kernel(i, j)``
element callable becomes an object with element access -- a bound ``DenseOp`` / ``KernelGramOp`` (``op.bind(...)``), a
dense matrix, or ``without_noise(bound_gram_op)`` for the noise-free kernel of likelihood_pdf_p
(util/gp_util.py:253-254).  Like the reference (low_rank.py:47-55,86-93), nothing here is differentiable.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .operators import BoundOp, DenseOp, NativeOp


class without_noise:
    """Marks a bound kernel-Gram operator as 'kernel only': K(X, X) without the noise on its diagonal."""

    def __init__(self, bound):
        self.bound = bound


def _element_source(lazy_kernel):
    with_noise = True
    if isinstance(lazy_kernel, without_noise):
        lazy_kernel, with_noise = lazy_kernel.bound, False
    if torch.is_tensor(lazy_kernel):
        lazy_kernel = DenseOp().bind(lazy_kernel)
    if not (isinstance(lazy_kernel, BoundOp) and isinstance(lazy_kernel.op, NativeOp)):
        raise TypeError("lazy_kernel must be a dense matrix or a bound DenseOp / KernelGramOp (element access on the "
                        "device); arbitrary (i, j) callables are not supported in the MI355X build")
    return lazy_kernel, with_noise


def _factor(lazy_kernel, n, rank, pivot):
    if rank > n:
        raise ValueError(f"Rank exceeds n: {rank} >= {n}.")
    if rank < 1:
        raise ValueError(f"Rank must be positive, but {rank} < {1}.")
    bound, with_noise = _element_source(lazy_kernel)
    with torch.no_grad():
        cparams = tuple(q.detach() for q in bound.op.constrain(*bound.params))
        _lib.require_device(*cparams)
        ref = cparams[0]
        dt, dev = ref.dtype, ref.device
        if bound.op.size(*cparams) != n:
            raise ValueError(f"operator has {bound.op.size(*cparams)} rows, expected n = {n}")
        desc = bound.op.descriptor(cparams, dt, n)
        ws = _lib.workspace_pcg(desc, n, 1, rank, dev)
        lt = torch.empty((rank, n), dtype=dt, device=dev)
        pivots = torch.empty((rank,), dtype=torch.int64, device=dev)
        success = torch.empty((1,), dtype=torch.int32, device=dev)
        _lib.check(_lib.get().mfx_partial_cholesky(C.byref(desc), rank, int(pivot), int(with_noise), _lib.ptr(lt),
                                                   _lib.ptr(pivots), _lib.ptr(success), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_ptr(dev)))
    return lt, pivots, success


def cholesky_partial(*, rank: int):
    """low_rank.py:63-120."""

    def cholesky(lazy_kernel, n: int, /):
        lt, _piv, _ok = _factor(lazy_kernel, n, rank, pivot=False)
        return lt.t(), {}

    return cholesky


def cholesky_partial_pivot(*, rank: int):
    """low_rank.py:123-228 (rows returned in the original order, :227-228)."""

    def cholesky(matrix_element, n: int):
        lt, piv, ok = _factor(matrix_element, n, rank, pivot=True)
        return lt.t(), {"success": ok[0] != 0, "pivots": piv}

    return cholesky


class _NoGrad(torch.autograd.Function):
    """low_rank.py:47-55: 'Ensure that no one ever differentiates through here'."""

    @staticmethod
    def forward(ctx, pre, v, s):
        return pre._apply(v, s)

    @staticmethod
    def backward(ctx, _g):
        raise RuntimeError


class _NoGradInvSqrt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre, v, s):
        return pre._apply_inv_sqrt(v, s)

    @staticmethod
    def backward(ctx, _g):
        raise RuntimeError


class Preconditioner:
    """solve(v, s) = (s I + L L^T)^{-1} v by the Woodbury identity (low_rank.py:31-43)."""

    def __init__(self, chol):
        lt = chol.t()
        self.lt = lt if lt.is_contiguous() else lt.contiguous()  # (rank, n); a view of what the factorisation wrote
        self.rank, self.n = self.lt.shape
        assert self.rank <= self.n, (self.n, self.rank)  # tall, not wide (low_rank.py:26-29)
        self._gram = None
        self._eig = None

    def inv_sqrt(self, s):
        """P^-1/2 = scale (I - L mid L^T) for P = s I + L L^T -> (mid (rank, rank) in the dtype of L, scale (1,) = s^-1/2).  With
        L^T L = V diag(g) V^T (fp64, the Gram matrix ``minv`` caches, g clamped at 0): mid = V diag(c) V^T,
        c_i = 1 / ((s + g_i) + sqrt(s (s + g_i))) -- the form without cancellation as g_i -> 0.  Not differentiable (``_NoGrad``
        convention); works on CPU tensors like ``minv``."""
        with torch.no_grad():
            if self._gram is None:
                self._gram = (self.lt @ self.lt.t()).double()
            if self._eig is None:
                gamma, vecs = torch.linalg.eigh(self._gram)
                self._eig = (gamma.clamp_min(0.0), vecs)
            gamma, vecs = self._eig
            s = torch.as_tensor(s, dtype=torch.float64, device=self.lt.device).detach().reshape(1)
            c = 1.0 / ((s + gamma) + torch.sqrt(s * (s + gamma)))
            mid = (vecs * c) @ vecs.t()
            mid = 0.5 * (mid + mid.t())
            return mid.to(self.lt.dtype).contiguous(), torch.rsqrt(s).to(self.lt.dtype).contiguous()

    def _apply_inv_sqrt(self, v, s):
        V = (v if v.dim() == 2 else v[None]).detach().contiguous()
        p, n = V.shape
        if n != self.n or V.dtype != self.lt.dtype:
            raise ValueError(f"preconditioner of size {self.n} ({self.lt.dtype}) applied to {tuple(v.shape)} ({v.dtype})")
        mid, scale = self.inv_sqrt(s)
        if not V.is_cuda:  # host tensors (tests of the formula): the same expression in torch
            z = scale * (V - ((V @ self.lt.t()) @ mid) @ self.lt)
            return z if v.dim() == 2 else z[0]
        lib, code = _lib.get(), _lib.dtype_code(V.dtype)
        ws = _lib.scratch(int(lib.mfx_lowrank_workspace_bytes(code, n, self.rank, p)), V.device)
        z = torch.empty_like(V)
        _lib.check(lib.mfx_lowrank_apply(code, n, self.rank, _lib.ptr(self.lt), _lib.ptr(mid), _lib.ptr(scale), _lib.ptr(V), n,
                                         _lib.ptr(z), n, p, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(V.device)))
        return z if v.dim() == 2 else z[0]

    def apply_inv_sqrt(self, v, s):
        """P^-1/2 v on (n,) or (p, n) by ``mfx_lowrank_apply``; not differentiable (``_NoGrad`` convention)."""
        if torch.is_grad_enabled() and (v.requires_grad or (torch.is_tensor(s) and s.requires_grad)):
            s_t = s if torch.is_tensor(s) else torch.as_tensor(s, dtype=v.dtype, device=v.device)
            return _NoGradInvSqrt.apply(self, v, s_t)
        return self._apply_inv_sqrt(v, s)

    def minv(self, s):
        """(s I + L^T L)^{-1} (rank, rank) and the device scalar s."""
        if self._gram is None:
            self._gram = (self.lt @ self.lt.t()).double()
        s = torch.as_tensor(s, dtype=self.lt.dtype, device=self.lt.device).detach().reshape(1)
        cap = self._gram + s.double() * torch.eye(self.rank, dtype=torch.float64, device=self.lt.device)
        minv = torch.cholesky_inverse(torch.linalg.cholesky(cap))
        return minv.to(self.lt.dtype).contiguous(), s.contiguous()

    def logdet(self, s):
        """log det(s I + L L^T) = (n - rank) log s + log det(s I_r + L^T L) (the matrix determinant lemma), from the fp64 Gram matrix
        that ``minv`` caches -> fp64 scalar on the device of L.  Not differentiable (``_NoGrad`` convention)."""
        if self._gram is None:
            self._gram = (self.lt @ self.lt.t()).double()
        s = s.detach() if torch.is_tensor(s) else torch.tensor(float(s), dtype=torch.float64)  # (a Python float is not rounded to fp32)
        s = s.to(self.lt.device).double().reshape(())
        cap = self._gram + s * torch.eye(self.rank, dtype=torch.float64, device=self.lt.device)
        return (self.n - self.rank) * torch.log(s) + 2.0 * torch.log(torch.diagonal(torch.linalg.cholesky(cap))).sum()

    def sample(self, seed, num, s, first_probe=0):
        """``num`` probes z (num, n) with E[z z^T] = s I + L L^T exactly: z = sqrt(s) e_1 + L e_2 with (e_1, e_2) the +-1 probe of
        length n + rank that ``mfx_rademacher`` draws for (seed, first_probe + b) -- one fused kernel (``mfx_precond_sample``).
        Shards with different ``first_probe`` tile one probe matrix."""
        _lib.require_device(self.lt)
        dt, dev = self.lt.dtype, self.lt.device
        sdev = torch.as_tensor(s, dtype=dt, device=dev).detach().reshape(1).contiguous()
        out = torch.empty((int(num), self.n), dtype=dt, device=dev)
        _lib.check(_lib.get().mfx_precond_sample(_lib.dtype_code(dt), self.n, self.rank, _lib.ptr(self.lt), _lib.ptr(sdev),
                                                 int(seed) & ((1 << 64) - 1), int(first_probe), int(num), _lib.ptr(out),
                                                 _lib.stream_ptr(dev)))
        return out

    def _apply(self, v, s):
        _lib.require_device(v)
        V = (v if v.dim() == 2 else v[None]).detach().contiguous()
        p, n = V.shape
        if n != self.n or V.dtype != self.lt.dtype:
            raise ValueError(f"preconditioner of size {self.n} ({self.lt.dtype}) applied to {tuple(v.shape)} ({v.dtype})")
        minv, sdev = self.minv(s)
        desc = _lib.Operator()
        desc.kind, desc.dtype, desc.n = _lib.OP_DENSE, _lib.dtype_code(V.dtype), n
        ws = _lib.workspace_pcg(desc, n, p, self.rank, V.device)
        z = torch.empty_like(V)
        _lib.check(_lib.get().mfx_precond_apply(desc.dtype, n, self.rank, _lib.ptr(self.lt), _lib.ptr(minv),
                                                _lib.ptr(sdev), _lib.ptr(V), n, _lib.ptr(z), n, p, _lib.ptr(ws),
                                                ws.numel(), _lib.stream_ptr(V.device)))
        return z if v.dim() == 2 else z[0]

    def __call__(self, v, s):
        if torch.is_grad_enabled() and (v.requires_grad or (torch.is_tensor(s) and s.requires_grad)):
            s_t = s if torch.is_tensor(s) else torch.as_tensor(s, dtype=v.dtype, device=v.device)
            return _NoGrad.apply(self, v, s_t)
        return self._apply(v, s)

    def bind(self, s):
        """P = lambda v: pre(v, s) (util/gp_util.py:265) in a form the native PCG loop recognises."""
        return BoundPreconditioner(self, s)


class BoundPreconditioner:
    def __init__(self, pre, s):
        self.pre, self.s = pre, s

    def __call__(self, v):
        return self.pre(v, self.s)

    def logdet(self):
        return self.pre.logdet(self.s)

    def inv_sqrt(self):
        return self.pre.inv_sqrt(self.s)

    def apply_inv_sqrt(self, v):
        return self.pre.apply_inv_sqrt(v, self.s)

    def sample(self, seed, num, first_probe=0):
        return self.pre.sample(seed, num, self.s, first_probe=first_probe)


def preconditioner(cholesky, /):
    """low_rank.py:10-60."""

    def solve_with_preconditioner(lazy_kernel, /, nrows: int):
        chol, info = cholesky(lazy_kernel, nrows)
        return Preconditioner(chol), info

    return solve_with_preconditioner
