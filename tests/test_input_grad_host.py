"""CPU-side checks of the input gradient of the kernel-Gram operator (no GPU): the `x` field of `mfx_op_grads`, the
refusals of the C-ABI before any launch, and what `RbfGramOp.constrain` hands to the autograd Functions."""

import ctypes
import os
import re

import pytest
import torch

from matfree_extensions import _lib, arnoldi
from matfree_extensions.operators import RbfGramOp, RowShardedOp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_op_grads_ends_in_x_and_the_ctypes_mirror_follows():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    gbody = header[header.index("typedef struct mfx_op_grads {") : header.index("} mfx_op_grads;")]
    fields = re.findall(r"\b(\w+);", gbody)
    assert fields[-1] == "x"
    assert [f[0] for f in _lib.OpGrads._fields_] == fields
    assert ctypes.sizeof(_lib.OpGrads) == len(fields) * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.OpGrads.x.offset == (len(fields) - 1) * ctypes.sizeof(ctypes.c_void_p)


def _rbf_desc(n=256, d=3, nrows=0):
    desc = _lib.Operator()
    desc.kind, desc.dtype, desc.n = _lib.OP_RBF, _lib.MFX_F32, n
    desc.x = desc.lengthscale = desc.outputscale = desc.noise = 64  # never dereferenced: the refusals come first
    desc.d, desc.ard = d, 0
    desc.row0, desc.nrows = 0, nrows
    return desc


def _grads_with_x():
    g = _lib.OpGrads()
    g.lengthscale = g.outputscale = g.noise = g.x = 64
    return g


def test_input_gradient_refusals_come_before_any_launch():
    lib = _lib.get()
    fake = ctypes.c_void_p(64)  # a pointer no kernel may touch: every call below must return before a launch
    g = _grads_with_x()
    # a non-Gram operator: MFX_ERR_INVALID
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n, dense.dense_a, dense.lda = _lib.OP_DENSE, _lib.MFX_F32, 4, 64, 4
    assert lib.mfx_op_vjp_params(ctypes.byref(dense), fake, 4, fake, 4, 1, ctypes.byref(g), fake, 1 << 20, None) == -1
    assert "kernel-Gram" in lib.mfx_last_error().decode()
    assert lib.mfx_lanczos_adjoint(ctypes.byref(dense), 4, 2, 1, fake, fake, fake, fake, None, fake, fake, fake, fake,
                                   ctypes.byref(g), fake, 0, None) == -1
    assert lib.mfx_arnoldi_adjoint(ctypes.byref(dense), 4, 2, 1, fake, fake, fake, fake, None, fake, None, None, 1, fake, fake,
                                   ctypes.byref(g), fake, 0, None) == -1
    # a row block of a Gram operator: MFX_ERR_UNSUPPORTED
    rows = _rbf_desc(nrows=64)
    assert lib.mfx_op_vjp_params(ctypes.byref(rows), fake, 64, fake, 256, 1, ctypes.byref(g), fake, 1 << 20, None) == -2
    assert "row" in lib.mfx_last_error().decode()
    # the row-sharded drivers: MFX_ERR_UNSUPPORTED, even on the whole operator
    whole = _rbf_desc()
    cm = _lib.Comm()
    cm.rank, cm.world, cm.nloc = 0, 1, 256
    assert lib.mfx_lanczos_adjoint_sharded(ctypes.byref(whole), ctypes.byref(cm), 256, 2, 1, fake, fake, fake, fake, None, fake,
                                           fake, fake, fake, fake, ctypes.byref(g), fake, 0, None) == -2
    assert lib.mfx_arnoldi_adjoint_sharded(ctypes.byref(whole), ctypes.byref(cm), 256, 2, 1, fake, fake, fake, fake, fake, None,
                                           fake, None, None, 1, fake, fake, ctypes.byref(g), fake, 0, None) == -2


def test_constrain_returns_three_tensors_unless_x_requires_grad():
    X = torch.randn(10, 3, dtype=torch.float64)
    raw = (torch.zeros(3, dtype=torch.float64), torch.tensor(0.1, dtype=torch.float64), torch.tensor(-1.0, dtype=torch.float64))
    plain = RbfGramOp(X).constrain(*raw)
    assert len(plain) == 3
    Xg = X.clone().requires_grad_(True)
    op = RbfGramOp(Xg)
    cp = op.constrain(*raw)
    assert len(cp) == 4 and cp[3] is op.X
    assert len(RbfGramOp(Xg.detach()).constrain(*raw)) == 3
    for a, b in zip(plain, cp[:3]):
        assert torch.equal(a, b)
    # the gradient tuple lines up with the constrained tensors; the X slot is (n, d) in X's dtype and wired into `x`
    st, g = op.new_grads(*cp)
    assert len(g) == 4 and g[3].shape == X.shape and g[3].dtype == X.dtype and st.x == g[3].data_ptr()
    st, g = RbfGramOp(X).new_grads(*plain)
    assert len(g) == 3 and st.x is None


def test_row_sharded_operator_refuses_an_x_that_requires_grad():
    Xg = torch.randn(128, 2).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        RowShardedOp(RbfGramOp(Xg), comm=None)


def test_complex_arnoldi_refuses_an_x_that_requires_grad():
    Xg = torch.randn(8, 2, dtype=torch.float64).requires_grad_(True)
    raw = (torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))
    v = torch.ones(8, dtype=torch.complex128)
    with pytest.raises(NotImplementedError, match="forward only"):
        arnoldi.hessenberg(RbfGramOp(Xg), 2, reortho="full")(v, *raw)
