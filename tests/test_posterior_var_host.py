"""CPU-side checks of the GP predictive variance (no GPU): the dense-weight cross VJP is declared, mirrored in ctypes and exported,
every refusal of mfx_gram_cross_vjp_dense comes back with its code and message before any launch, and the Python layer refuses
bad chunks, bad test points, kernels that are not native and row-sharded operators."""

import ctypes

import os

import pytest
import torch

from matfree_extensions import _lib, cg
from matfree_extensions.operators import RbfGramOp, RowShardedOp
from matfree_extensions.util import gp_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfx_gram_cross_vjp_dense_workspace_bytes", "mfx_gram_cross_vjp_dense")
FAKE = ctypes.c_void_p(64)  # a device pointer no kernel may touch: every call below must return before a launch
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


def test_new_symbols_are_declared_mirrored_and_exported():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.get()
    for name in NEW:
        assert f" {name}(" in header, name
        assert name in _lib.SYMBOLS, name
        assert name in integration, name
        assert getattr(lib, name) is not None
    assert lib.mfx_version() == 201


def _rbf(n=300, d=3, nrows=0, dtype=_lib.MFX_F32):
    desc = _lib.Operator()
    desc.kind, desc.dtype, desc.n = _lib.OP_RBF, dtype, n
    desc.x = desc.lengthscale = desc.outputscale = desc.noise = 64
    desc.d, desc.ard = d, 0
    desc.row0, desc.nrows = 0, nrows
    return desc


def _grads(**fields):
    g = _lib.OpGrads()
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def _dense(desc, m=7, lds=None, grads=None, ws_bytes=1 << 30, ws=FAKE, xnew=FAKE, S=FAKE):
    lds = desc.n if lds is None else lds
    grads = _grads(lengthscale=64, outputscale=64, x=64) if grads is None else grads
    return _lib.get().mfx_gram_cross_vjp_dense(ctypes.byref(desc), xnew, m, S, lds, ctypes.byref(grads), FAKE, ws, ws_bytes, None)


def _err():
    return _lib.get().mfx_last_error().decode()


def test_workspace_query():
    lib = _lib.get()
    desc = _rbf()
    assert lib.mfx_gram_cross_vjp_dense_workspace_bytes(ctypes.byref(desc), 16) == lib.mfx_gram_cross_vjp_workspace_bytes(
        ctypes.byref(desc), 16, 1)
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n = _lib.OP_DENSE, _lib.MFX_F32, 4
    assert lib.mfx_gram_cross_vjp_dense_workspace_bytes(ctypes.byref(dense), 16) == -1
    assert lib.mfx_gram_cross_vjp_dense_workspace_bytes(ctypes.byref(desc), 0) == -1


def test_non_gram_operator_is_unsupported():
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n, dense.dense_a, dense.lda = _lib.OP_DENSE, _lib.MFX_F32, 4, 64, 4
    assert _dense(dense, grads=_grads(outputscale=64)) == UNSUPPORTED and "kernel-Gram" in _err()


def test_row_blocks_are_unsupported():
    assert _dense(_rbf(nrows=64)) == UNSUPPORTED and "row block" in _err()


@pytest.mark.parametrize("kw", [dict(m=0), dict(lds=299), dict(xnew=None), dict(S=None)])
def test_bad_sizes_and_nulls_are_invalid(kw):
    assert _dense(_rbf(), **kw) == INVALID
    assert "mfx_gram_cross_vjp_dense" in _err()


def test_a_null_grads_struct_is_invalid():
    desc = _rbf()
    assert _lib.get().mfx_gram_cross_vjp_dense(ctypes.byref(desc), FAKE, 7, FAKE, 300, None, FAKE, FAKE, 1 << 30, None) == INVALID


@pytest.mark.parametrize("field", ["dense_a", "val"])
def test_fields_of_other_operators_are_invalid(field):
    assert _dense(_rbf(), grads=_grads(**{field: 64, "outputscale": 64})) == INVALID
    assert "dense_a / val" in _err()


def test_null_operator_data_is_invalid():
    desc = _rbf()
    desc.x = None
    assert _dense(desc) == INVALID and "null" in _err()


def test_short_workspace_is_refused():
    lib = _lib.get()
    desc = _rbf(n=4096, d=8)
    need = lib.mfx_gram_cross_vjp_dense_workspace_bytes(ctypes.byref(desc), 7)
    assert _dense(desc, ws_bytes=need - 512) == WORKSPACE and "workspace" in _err()
    assert _dense(desc, ws=None) == WORKSPACE


# ---- Python refusals (raised before any device work, so CPU tensors suffice) ----------------------------------------------------

def _op_params(d=3):
    X = torch.zeros(10, d)
    return RbfGramOp(X), (torch.zeros(()), torch.zeros(()), torch.zeros(()))


@pytest.mark.parametrize("chunk", [0, -3])
def test_posterior_variance_refuses_a_bad_chunk(chunk):
    op, params = _op_params()
    with pytest.raises(ValueError, match="chunk"):
        op.posterior_variance(torch.zeros(4, 3), cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=10), *params, chunk=chunk)


@pytest.mark.parametrize("shape", [(4, 2), (4,), (0, 3)])
def test_posterior_variance_refuses_bad_test_points(shape):
    op, params = _op_params()
    with pytest.raises(ValueError, match="xs"):
        op.posterior_variance(torch.zeros(shape), cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=10), *params)


def test_likelihood_condition_var_refuses_a_bad_chunk():
    constrain = gp_util.constraint_greater_than(1e-4)
    with pytest.raises(ValueError, match="chunk"):
        gp_util.likelihood_condition_var(gp_util.gram_matvec(), cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=10), constrain=constrain,
                                         chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        gp_util.likelihood_condition_var_p(gp_util.gram_matvec(), cg.pcg_adaptive(atol=1e-6, rtol=0.0, maxiter=10),
                                           precondition=None, constrain=constrain, chunk=0)


def test_likelihood_condition_var_refuses_a_kernel_that_is_not_native():
    lik, _ = gp_util.likelihood_condition_var(gp_util.gram_matvec(), cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=10),
                                              constrain=gp_util.constraint_greater_than(1e-4))
    with pytest.raises(TypeError, match="native"):
        lik(torch.zeros(10, 3), lambda x: x.sum(), lambda x, y: (x * y).sum(), params={"raw_noise": torch.zeros(())})


def test_row_sharded_operators_refuse_the_variance():
    sharded = RowShardedOp.__new__(RowShardedOp)  # (a real one needs a process group; the refusal does not look at it)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        sharded.posterior_variance(torch.zeros(4, 3), None, torch.zeros(()), torch.zeros(()), torch.zeros(()))
