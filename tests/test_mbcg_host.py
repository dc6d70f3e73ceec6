"""CPU-side checks of modified batched CG (no GPU): the NumPy restatement of mfx_mbcg_solve's outputs (tests/_mbcg_restatement.py)
reproduces b^T M^-1/2 log(M^-1/2 A M^-1/2) M^-1/2 b against a dense eigendecomposition, through breakdown truncation; the
preconditioner's log-determinant is the dense one; the three new entry points are declared, mirrored in ctypes and exported, and refuse
bad arguments with their codes before any launch; the Python layer refuses row-sharded operators and foreign preconditioners.

Tolerances: SURVEY.md section 8(d) -- fp64 forward 1e-9 (the restatement itself is held to 1e-10 here), fp32 value 1e-4."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _mbcg_restatement as mb
from matfree_extensions import _lib, cg, low_rank
from matfree_extensions.operators import DenseOp, RowShardedOp
from matfree_extensions.util import gp_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)  # a device pointer no kernel may touch: every call below must return before a launch
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
NEW = ("mfx_mbcg_workspace_bytes", "mfx_mbcg_solve", "mfx_precond_sample")


def _restated_quadform(dtype, rank):
    X, (ls, os_, noise), A, L, M, R = mb.table_setting()
    n = len(X)
    if rank:
        Z = mb.probes_with_covariance(R, L, noise)
        precond = mb.woodbury(L, noise, dtype)
    else:
        Z, M, precond = R[:, :n].copy(), None, None
    x, r, steps, rzs, paps, w0 = mb.pcg(A.astype(dtype), Z.astype(dtype), precond, n)
    tdiag, toff, depth = mb.tridiag(rzs, paps, steps, n)
    return mb.quadrature(tdiag, toff, rzs[:, 0]), mb.dense_quadform(A, M, Z), depth, (tdiag, toff)


@pytest.mark.parametrize("rank", [0, 8])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-4)])
def test_restatement_reproduces_the_dense_quadratic_form(dtype, tol, rank):
    got, want, depth, (tdiag, toff) = _restated_quadform(dtype, rank)
    err = np.abs(got - want) / np.abs(want)
    print(f"{np.dtype(dtype).name} rank {rank}: relative errors {err}, depth {depth}")
    assert np.all(err <= tol), (err, depth)
    n = tdiag.shape[1]
    assert np.all(depth >= 1) and np.all(depth <= n)
    if rank or dtype is np.float32:  # these runs break down before n steps: the live block is truncated (fp64 without a preconditioner is not)
        assert np.all(depth < n), depth
    for b, m in enumerate(depth):  # the padding is exactly the identity block
        assert np.all(tdiag[b, m:] == 1) and np.all(toff[b, max(m - 1, 0):] == 0)
        assert np.all(tdiag[b, :m] > 0) and np.all(toff[b, : m - 1] > 0)


def test_zero_right_hand_side_has_depth_zero_and_the_identity_tridiagonal():
    A = mb.table_setting()[2]
    B = np.zeros((2, len(A)))
    B[1] = 1.0
    x, r, steps, rzs, paps, w0 = mb.pcg(A, B, None, 5)
    tdiag, toff, depth = mb.tridiag(rzs, paps, steps, 5)
    assert depth.tolist() == [0, 5] and np.all(tdiag[0] == 1) and np.all(toff[0] == 0) and np.all(x[0] == 0)
    assert mb.quadrature(tdiag, toff, rzs[:, 0])[0] == 0.0


def test_preconditioner_logdet_matches_the_dense_determinant():
    X, (ls, os_, noise), A, L, M, R = mb.table_setting()
    pre = low_rank.Preconditioner(torch.tensor(L, dtype=torch.float64))
    for s in (noise, 2.5):
        dense = s * torch.eye(len(X), dtype=torch.float64) + torch.tensor(L) @ torch.tensor(L).T
        sign, want = torch.linalg.slogdet(dense)
        got = pre.logdet(s)
        assert sign == 1 and got.dtype == torch.float64
        assert abs(got.item() - want.item()) <= 1e-10 * abs(want.item()), (got.item(), want.item())
        assert pre.bind(torch.tensor(s, dtype=torch.float64)).logdet().item() == got.item()


def test_new_symbols_are_declared_mirrored_and_exported():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.get()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(const", header) or re.search(r"\b" + name + r"\(int dtype", header), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
        assert name in integration, name
    flat = " ".join(header.split())
    decl = re.search(r"int mfx_mbcg_solve\(([^)]*)\);", flat).group(1).split(",")
    assert [a.split()[-1] for a in decl] == ["op", "b", "ldb", "n", "p", "precond_lt", "rank", "precond_minv", "precond_shift", "maxiter",
                                            "miniter", "atol", "rtol", "adaptive", "x", "r", "num_steps", "w0", "tdiag", "toff", "rz0",
                                            "depth", "ws", "ws_bytes", "stream"]
    assert len(_lib.SYMBOLS["mfx_mbcg_solve"][1]) == len(decl)
    decl = re.search(r"int mfx_precond_sample\(([^)]*)\);", flat).group(1).split(",")
    assert [a.split()[-1] for a in decl] == ["dtype", "n", "rank", "lt", "shift", "seed", "first_probe", "p", "out", "stream"]
    assert len(_lib.SYMBOLS["mfx_precond_sample"][1]) == len(decl)
    assert lib.mfx_version() == 201


def _dense(n=40, nrows=0):
    desc = _lib.Operator()
    desc.kind, desc.dtype, desc.n, desc.dense_a, desc.lda = _lib.OP_DENSE, _lib.MFX_F64, n, 64, n
    desc.row0, desc.nrows = 0, nrows
    return desc


def _mbcg(desc, n=40, p=3, maxiter=5, ws=FAKE, ws_bytes=1 << 30, **null):
    ptr = {k: FAKE for k in ("b", "x", "r", "steps", "w0", "tdiag", "toff", "rz0", "depth")}
    ptr.update(null)
    return _lib.get().mfx_mbcg_solve(ctypes.byref(desc), ptr["b"], n, n, p, None, 0, None, None, maxiter, 0, 1.0, 0.0, 0, ptr["x"],
                                     ptr["r"], ptr["steps"], ptr["w0"], ptr["tdiag"], ptr["toff"], ptr["rz0"], ptr["depth"], ws,
                                     ws_bytes, None)


@pytest.mark.parametrize("which", ["tdiag", "toff", "rz0", "depth"])
def test_mbcg_solve_requires_its_coefficient_outputs(which):
    assert _mbcg(_dense(), **{which: None}) == INVALID
    assert which in _lib.get().mfx_last_error().decode()


@pytest.mark.parametrize("maxiter", [0, -3])
def test_mbcg_solve_needs_an_iteration(maxiter):
    assert _mbcg(_dense(), maxiter=maxiter) == INVALID
    assert "maxiter" in _lib.get().mfx_last_error().decode()


def test_mbcg_solve_refuses_row_blocks_and_short_workspaces():
    assert _mbcg(_dense(nrows=16)) == UNSUPPORTED and "row block" in _lib.get().mfx_last_error().decode()
    lib = _lib.get()
    desc = _dense()
    need = lib.mfx_mbcg_workspace_bytes(ctypes.byref(desc), 40, 3, 0, 5)
    plain = lib.mfx_pcg_workspace_bytes(ctypes.byref(desc), 40, 3, 0)
    assert need >= plain - 1280 + 2 * 3 * 6 * 8  # the PCG vectors and the two (p, maxiter + 1) records
    assert _mbcg(desc, ws_bytes=need - 512) == WORKSPACE and "workspace" in lib.mfx_last_error().decode()
    assert _mbcg(desc, ws=None) == WORKSPACE
    assert lib.mfx_mbcg_workspace_bytes(ctypes.byref(desc), 40, 3, 0, 0) == -1
    assert lib.mfx_mbcg_workspace_bytes(None, 40, 3, 0, 5) == -1
    # w0 alone is optional: without it the call gets as far as the workspace check
    assert _mbcg(desc, w0=None, ws_bytes=0) == WORKSPACE


def test_precond_sample_refusals():
    lib = _lib.get()

    def sample(dtype=_lib.MFX_F64, n=10, rank=2, lt=FAKE, shift=FAKE, p=3, out=FAKE):
        return lib.mfx_precond_sample(dtype, n, rank, lt, shift, 7, 0, p, out, None)

    for kw in (dict(out=None), dict(n=0), dict(p=0), dict(rank=-1), dict(lt=None), dict(shift=None), dict(dtype=5)):
        assert sample(**kw) == INVALID, kw
    assert sample(rank=1025) == UNSUPPORTED


def test_python_layer_refuses_row_sharding_and_foreign_preconditioners():
    sharded = RowShardedOp.__new__(RowShardedOp)  # (a real one needs a process group; the refusal does not look at it)
    b = torch.ones(4)
    for solve in (cg.mbcg_fixed_step(3), cg.mbcg_adaptive(atol=1e-3, rtol=0.0, maxiter=5)):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            solve(sharded, b, None)
        with pytest.raises(TypeError, match="P must be None"):
            solve(DenseOp().bind(torch.eye(4)), b, lambda v: v)
        with pytest.raises(NotImplementedError, match="row-sharded"):
            gp_util.krylov_logdet_mbcg(solve, num_probes=2)(sharded, 0)
        with pytest.raises(TypeError, match="P must be None"):
            gp_util.logpdf_mbcg(solve, num_probes=2)(b, 0, mean=torch.zeros(4), cov_matvec=DenseOp().bind(torch.eye(4)), P=lambda v: v)
    with pytest.raises(TypeError, match="mbcg"):
        gp_util.logpdf_mbcg(cg.pcg_fixed_step(3), num_probes=2)
    with pytest.raises(ValueError, match="at least one"):
        cg.mbcg_fixed_step(0)(DenseOp().bind(torch.eye(4)), b, None)
    with pytest.raises(_lib.MfxError, match="no CPU fallback"):
        cg.mbcg_fixed_step(2)(DenseOp().bind(torch.eye(4)), b, None)
