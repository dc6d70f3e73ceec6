"""CPU-side checks of the dense Gram block and the joint GP predictive covariance (no GPU): mfx_gram_block and its workspace query are
declared, mirrored in ctypes with the declared prototypes and exported; every refusal of mfx_gram_block comes back with its code
before any launch (the descriptor and the arguments hold dummy pointers no kernel may touch); and the Python layer refuses bad
chunks, badly shaped points, bad sample counts and row-sharded operators before any device work.

(The symmetric block with a rectangular request -- xb == NULL with mb != ma -- can only be asked for through the C interface:
RbfGramOp.gram_block(xa, None) has no second size.  It is checked there, and the Python method is checked to refuse a second
point set of the wrong shape.)"""

import ctypes
import os
import re

import pytest
import torch

from matfree_extensions import _lib, cg
from matfree_extensions.operators import RbfGramOp, RowShardedOp
from matfree_extensions.util import gp_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)  # a device pointer no kernel may touch: every call below must return before a launch
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
_CTYPE = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}
PROTOTYPES = {
    "mfx_gram_block_workspace_bytes": ("int64_t", ["const mfx_operator*", "int64_t", "int64_t"]),
    "mfx_gram_block": ("int", ["const mfx_operator*", "const void*", "int64_t", "const void*", "int64_t", "void*", "int64_t", "void*",
                               "int64_t", "void*"]),
}


def _ctype(c_type):
    if c_type == "const mfx_operator*":
        return ctypes.POINTER(_lib.Operator)
    return ctypes.c_void_p if c_type.endswith("*") else _CTYPE[c_type]


def test_new_symbols_are_declared_mirrored_and_exported():
    header = " ".join(open(os.path.join(ROOT, "include", "mfx.h")).read().split())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.get()
    for name, (res, args) in PROTOTYPES.items():
        decl = re.search(r"(\w+) " + name + r"\(([^)]*)\);", header)
        assert decl is not None, name
        declared = [" ".join(a.split()[:-1]) for a in decl.group(2).split(",")]  # drop the parameter names
        assert (decl.group(1), declared) == (res, args), name
        assert _lib.SYMBOLS[name] == (_ctype(res), [_ctype(a) for a in args]), name
        fn = getattr(lib, name)
        assert fn.restype is _ctype(res) and list(fn.argtypes) == [_ctype(a) for a in args]
        assert name in integration, name
    assert lib.mfx_version() == 201


def _rbf(n=300, d=3, nrows=0, dtype=_lib.MFX_F32, kernel_fn=0):
    desc = _lib.Operator()
    desc.kind, desc.dtype, desc.n = _lib.OP_RBF, dtype, n
    desc.x = desc.lengthscale = desc.outputscale = desc.noise = 64
    desc.d, desc.ard, desc.kernel_fn = d, 0, kernel_fn
    desc.row0, desc.nrows = 0, nrows
    return desc


def _block(desc, ma=7, mb=5, ldo=None, xa=FAKE, xb=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 30):
    ldo = mb if ldo is None else ldo
    op = None if desc is None else ctypes.byref(desc)
    return _lib.get().mfx_gram_block(op, xa, ma, xb, mb, out, ldo, ws, ws_bytes, None)


def _err():
    return _lib.get().mfx_last_error().decode()


def test_workspace_query():
    lib = _lib.get()
    small, large = (lib.mfx_gram_block_workspace_bytes(ctypes.byref(_rbf(d=8)), m, m) for m in (64, 4096))
    assert 0 < small < large
    # the scaled points and the squared norms of both sets, each rounded up to the carve's 256 bytes
    assert large >= 2 * (4096 * 8 * 4 + 4096 * 4)
    assert lib.mfx_gram_block_workspace_bytes(ctypes.byref(_rbf(d=8, dtype=_lib.MFX_F64)), 4096, 4096) >= 2 * large - 4096
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n = _lib.OP_DENSE, _lib.MFX_F32, 4
    assert lib.mfx_gram_block_workspace_bytes(ctypes.byref(dense), 16, 16) == -1
    assert lib.mfx_gram_block_workspace_bytes(ctypes.byref(_rbf()), 0, 16) == -1
    assert lib.mfx_gram_block_workspace_bytes(ctypes.byref(_rbf()), 16, 0) == -1
    assert lib.mfx_gram_block_workspace_bytes(None, 16, 16) == -1


def test_non_gram_operator_is_unsupported():
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n, dense.dense_a, dense.lda = _lib.OP_DENSE, _lib.MFX_F32, 4, 64, 4
    assert _block(dense) == UNSUPPORTED and "kernel-Gram" in _err()


def test_row_blocks_are_unsupported():
    assert _block(_rbf(nrows=64)) == UNSUPPORTED and "row block" in _err()


@pytest.mark.parametrize("kw", [dict(xa=None), dict(out=None), dict(ma=0), dict(mb=0), dict(ma=-4), dict(mb=5, ldo=4)])
def test_nulls_and_bad_sizes_are_invalid(kw):
    assert _block(_rbf(), **kw) == INVALID
    assert "mfx_gram_block" in _err()


def test_a_null_operator_is_invalid():
    assert _block(None) == INVALID


@pytest.mark.parametrize("field", ["lengthscale", "outputscale"])
def test_null_hyper_parameters_are_invalid(field):
    desc = _rbf()
    setattr(desc, field, None)
    assert _block(desc) == INVALID and "null" in _err()


def test_the_operators_own_points_and_noise_are_not_needed():
    """op->x and op->noise are not read: a descriptor without them gets as far as the workspace check"""
    desc = _rbf()
    desc.x = desc.noise = None
    assert _block(desc, ws_bytes=0) == WORKSPACE


def test_the_symmetric_block_must_be_square():
    assert _block(_rbf(), ma=7, mb=5, xb=None) == INVALID and "symmetric" in _err()
    assert _block(_rbf(), ma=7, mb=7, xb=None, ws_bytes=0) == WORKSPACE  # square: accepted up to the workspace check


@pytest.mark.parametrize("kernel_fn", [-1, 4, 17])
def test_an_unknown_kernel_is_invalid(kernel_fn):
    assert _block(_rbf(kernel_fn=kernel_fn)) == INVALID and "kernel_fn" in _err()


@pytest.mark.parametrize("dtype", [-1, 2])
def test_an_unknown_dtype_is_invalid(dtype):
    assert _block(_rbf(dtype=dtype)) == INVALID and "dtype" in _err()


def test_too_wide_inputs_are_unsupported():
    assert _block(_rbf(d=1025)) == UNSUPPORTED and "1024" in _err()
    assert _block(_rbf(d=1024), ws_bytes=0) == WORKSPACE


def test_short_workspace_is_refused():
    lib = _lib.get()
    desc = _rbf(d=8)
    need = lib.mfx_gram_block_workspace_bytes(ctypes.byref(desc), 4096, 300)
    assert _block(desc, ma=4096, mb=300, ws_bytes=need - 512) == WORKSPACE and "workspace" in _err()
    assert _block(desc, ma=4096, mb=300, ws=None) == WORKSPACE


# ---- Python refusals (raised before any device work, so CPU tensors suffice) ----------------------------------------------------

def _op_params(d=3):
    X = torch.zeros(10, d)
    return RbfGramOp(X), (torch.zeros(()), torch.zeros(()), torch.zeros(()))


def _solver():
    return cg.cg_adaptive(atol=1e-6, rtol=0.0, maxiter=10)


@pytest.mark.parametrize("chunk", [0, -3])
def test_posterior_covariance_refuses_a_bad_chunk(chunk):
    op, params = _op_params()
    with pytest.raises(ValueError, match="chunk"):
        op.posterior_covariance(torch.zeros(4, 3), _solver(), *params, chunk=chunk)


@pytest.mark.parametrize("shape", [(4, 2), (4,), (0, 3)])
def test_posterior_covariance_refuses_bad_test_points(shape):
    op, params = _op_params()
    with pytest.raises(ValueError, match="xs"):
        op.posterior_covariance(torch.zeros(shape), _solver(), *params)


@pytest.mark.parametrize("shape", [(4, 2), (4,), (0, 3)])
def test_gram_block_refuses_badly_shaped_points(shape):
    op, params = _op_params()
    with pytest.raises(ValueError, match="xa"):
        op.gram_block(torch.zeros(shape), None, *params)
    with pytest.raises(ValueError, match="xb"):
        op.gram_block(torch.zeros(4, 3), torch.zeros(shape), *params)


def test_likelihood_condition_cov_refuses_a_bad_chunk():
    constrain = gp_util.constraint_greater_than(1e-4)
    with pytest.raises(ValueError, match="chunk"):
        gp_util.likelihood_condition_cov(gp_util.gram_matvec(), _solver(), constrain=constrain, chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        gp_util.likelihood_condition_cov_p(gp_util.gram_matvec(), cg.pcg_adaptive(atol=1e-6, rtol=0.0, maxiter=10),
                                           precondition=None, constrain=constrain, chunk=0)


@pytest.mark.parametrize("num", [0, -2])
def test_posterior_samples_refuses_a_bad_count(num):
    with pytest.raises(ValueError, match="num"):
        gp_util.posterior_samples(3, torch.zeros(4), torch.eye(4), num=num)


def test_posterior_samples_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="cov"):
        gp_util.posterior_samples(3, torch.zeros(4), torch.eye(5), num=2)


def test_row_sharded_operators_refuse_the_covariance():
    sharded = RowShardedOp.__new__(RowShardedOp)  # (a real one needs a process group; the refusal does not look at it)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        sharded.posterior_covariance(torch.zeros(4, 3), None, torch.zeros(()), torch.zeros(()), torch.zeros(()))
