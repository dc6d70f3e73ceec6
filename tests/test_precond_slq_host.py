"""Preconditioned SLQ, host side (no GPU): the inverse square root of the partial-Cholesky preconditioner on CPU tensors, and every
refusal of an MFX_OP_PRECOND descriptor (struct mfx_precond behind ctx) through the C ABI (check_op runs before any launch: fake pointers, a huge ws_bytes).

inv_sqrt is compared with its definition, restated here: S = scale (I - L mid L^T) must satisfy S P S = I and S S = P^-1 for
P = s I + L L^T.  "To 1e-12" is relative to the largest entry of the right-hand side (1 for the identity; up to 1 / s = 1e4 for
P^-1, whose entries an fp64 S cannot carry to 1e-12 absolute), and the products are formed in extended precision from the fp64
S under test: at s = 1e-4 the entries of S reach 100 and those of P 40, so an fp64 evaluation of S P S alone leaves 4e-11 of its own
round-off (measured: 3.5e-11), which says nothing about S."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from matfree_extensions import _lib, low_rank, operators

N = 64
FAKE = ctypes.c_void_p(64)  # never dereferenced
BIG = 1 << 40
LD = np.longdouble


def _factor(n, r, zero_column):
    g = torch.Generator().manual_seed(100 * n + r)
    L = torch.randn((n, r), dtype=torch.float64, generator=g)
    if zero_column:
        L[:, r // 2] = 0.0  # one eigenvalue of L^T L exactly 0
    return L


@pytest.mark.parametrize("s", [1e-4, 0.1, 10.0])
@pytest.mark.parametrize("r,zero_column", [(1, False), (7, False), (7, True), (1, True)])
def test_inv_sqrt_is_the_inverse_square_root(r, zero_column, s):
    n = 40
    L = _factor(n, r, zero_column)
    pre = low_rank.Preconditioner(L)
    mid, scale = pre.inv_sqrt(s)
    assert mid.shape == (r, r) and mid.dtype == L.dtype and scale.shape == (1,) and not mid.requires_grad
    assert torch.equal(mid, mid.t())
    Lx, eye = L.numpy().astype(LD), np.eye(n, dtype=LD)
    S = scale.numpy().astype(LD)[0] * (eye - Lx @ mid.numpy().astype(LD) @ Lx.T)
    P = LD(s) * eye + Lx @ Lx.T
    err_id = np.abs(S @ P @ S - eye).max()
    Pinv = np.linalg.inv(P.astype(np.float64)).astype(LD)
    Pinv = Pinv @ (2 * eye - P @ Pinv)  # one Newton step in extended precision
    err_inv = np.abs(S @ S - Pinv).max() / np.abs(Pinv).max()
    print(f"r={r} zero={zero_column} s={s}: |S P S - I| = {float(err_id):.2e}, |S S - P^-1| / |P^-1| = {float(err_inv):.2e}")
    assert err_id <= 1e-12 and err_inv <= 1e-12
    # apply_inv_sqrt on host tensors is the same map, on one vector and on a batch; bound forms agree
    v = torch.randn((3, n), dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    want = torch.as_tensor((v.numpy().astype(LD) @ S).astype(np.float64))
    assert torch.allclose(pre.apply_inv_sqrt(v, s), want, rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    assert torch.allclose(pre.apply_inv_sqrt(v[0], s), want[0], rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    bound = pre.bind(s)
    assert torch.equal(bound.inv_sqrt()[0], mid) and torch.equal(bound.apply_inv_sqrt(v), pre.apply_inv_sqrt(v, s))


def test_inv_sqrt_is_not_differentiable():
    pre = low_rank.Preconditioner(_factor(40, 7, False))
    v = torch.randn(40, dtype=torch.float64, requires_grad=True)
    out = pre.apply_inv_sqrt(v, torch.tensor(0.1, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        out.sum().backward()
    s = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    assert not pre.inv_sqrt(s)[0].requires_grad and not pre.inv_sqrt(s)[1].requires_grad


def _dense(dtype=_lib.MFX_F64, n=N):
    d = _lib.Operator()
    d.kind, d.dtype, d.n, d.dense_a, d.lda = _lib.OP_DENSE, dtype, n, 64, n
    return d


def _precond(inner, dtype=_lib.MFX_F64, n=N, rank=3):
    d = _lib.Operator()
    d.kind, d.dtype, d.n = _lib.OP_PRECOND, dtype, n
    pc = _lib.Precond()
    pc.pc_inner = ctypes.addressof(inner) if inner is not None else None
    pc.pc_lt = pc.pc_mid = pc.pc_scale = 64
    pc.pc_rank = rank
    d.ctx, d.pc, d._keep = ctypes.addressof(pc), pc, inner
    return d


def _refusal_cases():
    none = _precond(_dense())
    none.ctx = None
    yield "NULL ctx", none, -1, "ctx (the mfx_precond) is NULL"
    yield "NULL inner", _precond(None), -1, "pc_inner is NULL"
    cb = _lib.Operator()
    cb.kind, cb.dtype, cb.n, cb.callback = _lib.OP_CALLBACK, _lib.MFX_F64, N, _lib.CALLBACK_T(lambda *a: 0)
    yield "inner CALLBACK", _precond(cb), -1, "must be native and not itself preconditioned"
    yield "inner PRECOND", _precond(_precond(_dense())), -1, "must be native and not itself preconditioned"
    own = _precond(_dense())
    own.pc.pc_inner = ctypes.addressof(own)  # a descriptor that names itself
    yield "inner PRECOND (itself)", own, -1, "must be native and not itself preconditioned"
    faulty = _dense()
    faulty.dense_a = None
    yield "inner refused by its own kind", _precond(faulty), -1, "dense operator without matrix"
    yield "dtype mismatch", _precond(_dense(_lib.MFX_F32)), -1, "dtype 1, inner operator 0"
    yield "n mismatch", _precond(_dense(n=N + 1)), -1, f"n = {N}, inner operator {N + 1}"
    yield "rank 0", _precond(_dense(), rank=0), -1, "rank 0 outside [1, n = 64]"
    yield "rank n + 1", _precond(_dense(), rank=N + 1), -1, f"rank {N + 1} outside [1, n = 64]"
    blocked = _dense()
    blocked.row0, blocked.nrows = 0, 32
    yield "inner row block", _precond(blocked), -1, "the inner operator must be whole"
    for field in ("pc_lt", "pc_mid", "pc_scale"):
        d = _precond(_dense())
        setattr(d.pc, field, None)
        yield f"NULL {field}", d, -1, "null factor"


def _entry_points(lib):
    F, ref = FAKE, ctypes.byref
    g = ref(_lib.OpGrads())
    pcg_tail = (None, 0, None, None, 3, 0, 0.0, 0.0, 0, F, F, None)
    return {
        "mfx_op_apply": lambda d: lib.mfx_op_apply(ref(d), F, N, F, N, 1, 0, F, BIG, None),
        "mfx_op_vjp_params": lambda d: lib.mfx_op_vjp_params(ref(d), F, N, F, N, 1, g, F, BIG, None),
        "mfx_lanczos_forward": lambda d: lib.mfx_lanczos_forward(ref(d), F, N, 2, 1, F, F, F, F, F, BIG, None),
        "mfx_lanczos_adjoint": lambda d: lib.mfx_lanczos_adjoint(ref(d), N, 2, 1, F, F, F, F, F, F, F, F, F, g, F, BIG, None),
        "mfx_arnoldi_forward": lambda d: lib.mfx_arnoldi_forward(ref(d), F, N, 2, 1, 1, F, F, F, F, F, BIG, None),
        "mfx_arnoldi_adjoint": lambda d: lib.mfx_arnoldi_adjoint(ref(d), N, 2, 1, F, F, F, F, F, F, F, F, _lib.REORTHO_NONE, F, F, g, F, BIG,
                                                              None),
        "mfx_pcg_solve": lambda d: lib.mfx_pcg_solve(ref(d), F, N, N, 1, *pcg_tail, F, BIG, None),
    }


def test_every_driver_refuses_a_faulty_preconditioned_descriptor_before_any_launch():
    lib = _lib.get()
    seen = 0
    for label, d, code, text in _refusal_cases():
        for name, call in _entry_points(lib).items():
            got = call(d)
            assert got == code and text in lib.mfx_last_error().decode(), (label, name, got, lib.mfx_last_error().decode())
            seen += 1
    assert seen == 14 * 7


def test_a_row_block_of_the_wrapper_is_refused():
    lib = _lib.get()
    d = _precond(_dense())
    d.row0, d.nrows = 0, 32
    assert lib.mfx_op_apply(ctypes.byref(d), FAKE, N, FAKE, N, 1, 0, FAKE, BIG, None) == -2
    assert "no row block" in lib.mfx_last_error().decode()
    assert lib.mfx_op_vjp_params(ctypes.byref(d), FAKE, N, FAKE, N, 1, ctypes.byref(_lib.OpGrads()), FAKE, BIG, None) == -2


def test_the_row_sharded_drivers_refuse_the_kind():
    lib = _lib.get()
    d = _precond(_dense())
    cm = _lib.Comm()
    cm.rank, cm.world, cm.nloc = 0, 1, N
    cm.allreduce_sum, cm.allgather = _lib.ALLREDUCE_T(lambda *a: 0), _lib.ALLGATHER_T(lambda *a: 0)
    F, ref = FAKE, ctypes.byref
    g = ref(_lib.OpGrads())
    calls = [
        lib.mfx_lanczos_forward_sharded(ref(d), ref(cm), F, N, 2, 1, F, F, F, F, F, BIG, None),
        lib.mfx_lanczos_adjoint_sharded(ref(d), ref(cm), N, 2, 1, F, F, F, F, F, F, F, F, F, F, g, F, BIG, None),
        lib.mfx_arnoldi_forward_sharded(ref(d), ref(cm), F, N, 2, 1, 1, F, F, F, F, F, F, BIG, None),
        lib.mfx_arnoldi_adjoint_sharded(ref(d), ref(cm), N, 2, 1, F, F, F, F, F, F, F, F, F, _lib.REORTHO_NONE, F, F, g, F, BIG, None),
        lib.mfx_pcg_solve_sharded(ref(d), ref(cm), F, N, N, 1, None, 0, None, None, 3, 0, 0.0, 0.0, 0, F, F, None, F, BIG, None),
    ]
    assert calls == [-2] * 5 and "row sharding a preconditioned operator is not implemented" in lib.mfx_last_error().decode()
    with pytest.raises(NotImplementedError, match="row sharding a PreconditionedOp"):
        operators.RowShardedOp(operators.PreconditionedOp(operators.DenseOp(), None, 0.1), None)


def test_one_specific_kind_sites_refuse_the_kind():
    """the element access of mfx_partial_cholesky and a Gram-only entry point refuse it as they refuse every other kind"""
    lib = _lib.get()
    d = _precond(_dense())
    assert lib.mfx_partial_cholesky(ctypes.byref(d), 2, 1, 1, FAKE, FAKE, FAKE, FAKE, BIG, None) < 0
    assert lib.mfx_gram_cross_apply(ctypes.byref(d), FAKE, 4, FAKE, N, FAKE, 4, 1, FAKE, BIG, None) == -2
    assert lib.mfx_gram_block_workspace_bytes(ctypes.byref(d), 4, 4) == -1


def test_gradient_fields_follow_the_inner_kind():
    """grads->x is the inner kind's to take: refused around a dense inner operator as on the dense operator itself"""
    lib = _lib.get()
    g = _lib.OpGrads()
    g.x = 64
    d = _precond(_dense())
    assert lib.mfx_op_vjp_params(ctypes.byref(d), FAKE, N, FAKE, N, 1, ctypes.byref(g), FAKE, BIG, None) == -1
    assert "needs a kernel-Gram operator" in lib.mfx_last_error().decode()


def test_lowrank_apply_refusals_and_workspace_size():
    lib = _lib.get()
    F = FAKE

    def call(dtype=_lib.MFX_F64, n=N, rank=3, lt=F, mid=F, scale=F, v=ctypes.c_void_p(1 << 20), ldv=N, z=ctypes.c_void_p(1 << 30), ldz=N,
             p=2, ws=F, nb=BIG):
        return lib.mfx_lowrank_apply(dtype, n, rank, lt, mid, scale, v, ldv, z, ldz, p, ws, nb, None)

    assert call(rank=0) == -1 and call(rank=N + 1) == -1
    assert call(lt=None) == -1 and call(mid=None) == -1 and call(scale=None) == -1 and call(v=None) == -1 and call(z=None) == -1
    assert call(p=0) == -1 and call(ldv=N - 1) == -1 and call(ldz=N - 1) == -1
    assert call(dtype=7) == -2
    assert call(n=8192, rank=4097, ldv=8192, ldz=8192) == -2
    # overlap: anything but Z == V with ldz == ldv
    base = 1 << 20
    assert call(v=ctypes.c_void_p(base), z=ctypes.c_void_p(base + 8)) == -1 and "overlaps" in lib.mfx_last_error().decode()
    assert call(v=ctypes.c_void_p(base), z=ctypes.c_void_p(base), ldz=N + 1) == -1
    assert call(v=ctypes.c_void_p(base), z=ctypes.c_void_p(base + 8 * (2 * N - 1))) == -1
    assert call(ws=None) == -4 and call(nb=255) == -4
    assert call(v=ctypes.c_void_p(base), z=ctypes.c_void_p(base), nb=255) == -4  # in place gets as far as the workspace
    # partials (p, rank, slices) and U (p, rank), each rounded up to 256 bytes; 512 (fp64) / 1024 (fp32) elements per slice
    assert lib.mfx_lowrank_workspace_bytes(_lib.MFX_F64, 1025, 3, 2) == 256 + 256
    assert lib.mfx_lowrank_workspace_bytes(_lib.MFX_F32, 4099, 33, 65) == 65 * 33 * 5 * 4 // 256 * 256 + 256 + 65 * 33 * 4 // 256 * 256 + 256
    assert lib.mfx_lowrank_workspace_bytes(_lib.MFX_F64, 64, 0, 1) == -1 and lib.mfx_lowrank_workspace_bytes(3, 64, 1, 1) == -1


def test_struct_and_python_surface():
    assert _lib.OP_PRECOND == 6
    # struct mfx_precond travels through ctx, as the GGN net does: mfx_operator does not grow, and the mirror follows the header
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfx.h")).read()
    body = header[header.index("typedef struct mfx_precond {") : header.index("} mfx_precond;")]
    assert re.findall(r"\b(\w+);", body) == [n for n, _ in _lib.Precond._fields_] == ["pc_inner", "pc_lt", "pc_mid", "pc_scale", "pc_rank"]
    assert ctypes.sizeof(_lib.Precond) == 5 * 8 and "pc_inner" not in [n for n, _ in _lib.Operator._fields_]
    assert re.search(r"enum \{ MFX_OP_PRECOND = 6 \}", header)
    op = operators.PreconditionedOp(operators.DenseOp(), low_rank.Preconditioner(_factor(40, 7, False)), torch.tensor(0.5, requires_grad=True))
    assert not op.s.requires_grad and op.kind == 6
    assert float(op.logdet()) == pytest.approx(float(torch.linalg.slogdet(0.5 * torch.eye(40, dtype=torch.float64)
                                                                          + op.pre.lt.t() @ op.pre.lt)[1]), rel=1e-12)
    with pytest.raises(TypeError):
        operators.PreconditionedOp(op, op.pre, 0.5)
    with pytest.raises(TypeError):
        operators.PreconditionedOp(lambda v: v, op.pre, 0.5)


def test_a_descriptor_keeps_the_constrained_parameters_alive():
    """op.descriptor(op.constrain(*params), ...) is the only owner of the tensors constrain returns: the descriptor must hold them, or
    the allocator reuses their memory for the caller's next tensor while the descriptor still points at it."""
    import gc
    import weakref

    X = torch.randn((16, 3), dtype=torch.float64)
    op = operators.RbfGramOp(X)
    raw = [torch.tensor(v, dtype=torch.float64) for v in (0.9, 0.4, -1.0)]
    cparams = op.constrain(*raw)
    refs = [weakref.ref(t) for t in cparams]
    desc = op.descriptor(cparams, torch.float64, 16)
    del cparams
    gc.collect()
    assert all(r() is not None for r in refs)
    assert (desc.lengthscale, desc.outputscale, desc.noise) == tuple(r().data_ptr() for r in refs)
    pop = operators.PreconditionedOp(operators.DenseOp(), low_rank.Preconditioner(_factor(16, 3, False)), 0.5)
    A = torch.randn((16, 16), dtype=torch.float64)
    inner_keep = weakref.ref(A)
    with pytest.raises(_lib.MfxError):  # (the factor must be on the device; the inner descriptor is built before that is looked at)
        pop.descriptor((A,), torch.float64, 16)
    assert inner_keep() is A
