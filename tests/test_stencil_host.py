"""CPU-side checks of the matrix-free 3x3 stencil operator (no GPU): the descriptor mirror, the NumPy restatement that the GPU tests
measure against (tied to the assembled CSR wave operator and to scipy's convolve2d), the transpose rule, and the refusals of the
C-ABI, which all come before any launch (the descriptor's pointers are never dereferenced)."""

import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal
import torch

import _stencil_restatement as sr
from matfree_extensions import _lib
from matfree_extensions.operators import RowShardedOp, StencilOp
from matfree_extensions.util import pde_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FIELDS = ["st_ny", "st_nx", "st_form", "st_boundary", "st_w"]


def test_descriptor_mirror_follows_the_header_and_ends_in_the_stencil_fields():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    body = header[header.index("typedef struct mfx_operator {") : header.index("} mfx_operator;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+);", body)
    names = [f[0] for f in _lib.Operator._fields_]
    assert names == fields
    assert names[-len(NEW_FIELDS) :] == NEW_FIELDS and names[-len(NEW_FIELDS) - 1] == "nrows"
    O = _lib.Operator
    assert O.st_ny.offset == O.nrows.offset + 8 and O.st_w.offset == O.st_ny.offset + 16
    assert ctypes.sizeof(O) == O.st_w.offset + 9 * 8
    assert re.search(r"typedef double mfx_stencil_weights\[9\];", header)
    values = dict(re.findall(r"(MFX_(?:OP|STENCIL|BOUNDARY)_[A-Z0-9]+) = (\d+)", header))
    assert values["MFX_OP_STENCIL"] == "4" == str(_lib.OP_STENCIL)
    assert (values["MFX_STENCIL_HEAT"], values["MFX_STENCIL_HEAT2"], values["MFX_STENCIL_WAVE"]) == ("0", "1", "2")
    assert (_lib.STENCIL_HEAT, _lib.STENCIL_HEAT2, _lib.STENCIL_WAVE) == (0, 1, 2)
    assert (values["MFX_BOUNDARY_DIRICHLET"], values["MFX_BOUNDARY_NEUMANN"]) == ("0", "1")
    assert (_lib.BOUNDARY_DIRICHLET, _lib.BOUNDARY_NEUMANN) == (0, 1)


@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
@pytest.mark.parametrize("res", [5, 16])
def test_restated_laplacian_wave_matrix_is_the_assembled_csr_one(res, boundary):
    """pde_util.wave_operator already reproduces the reference's targets (tests/test_gpu_next_tier.py, test_golden_fixtures): the
    new yardstick has to give the same matrix."""
    dx = 0.25
    rng = np.random.default_rng(res)
    coef = rng.uniform(0.5, 1.5, (res, res))
    op, values_fn = pde_util.wave_operator(res, dx, boundary=boundary, device="cpu")
    vals = values_fn(torch.tensor(coef)).numpy()
    n = 2 * res * res
    A = np.zeros((n, n))
    crow, col = op.crow.numpy(), op.col.numpy()
    for r in range(n):
        for e in range(crow[r], crow[r + 1]):
            A[r, col[e]] += vals[e]
    want = sr.dense_matrix("wave", pde_util.stencil_laplacian(dx).numpy(), boundary, coef, res, res)
    assert np.abs(A - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
def test_orientation_on_an_asymmetric_stencil_is_convolve2d(boundary):
    st = pde_util.stencil_advection_diffusion(0.5).numpy()
    assert not np.array_equal(st, st[::-1, ::-1])
    rng = np.random.default_rng(1)
    u = rng.standard_normal((4, 6))
    padded = np.pad(u, 1, mode="edge") if boundary == "neumann" else np.pad(u, 1)
    want = scipy.signal.convolve2d(st, padded, mode="valid")
    assert np.allclose(sr.conv(st, u, boundary), want, rtol=1e-14, atol=1e-14)
    # the pad callables of pde_util are the same padding, and carry their kind
    pad = pde_util.boundary_neumann() if boundary == "neumann" else pde_util.boundary_dirichlet()
    assert pad.kind == boundary and np.array_equal(pad(torch.tensor(u)).numpy(), padded)
    # StencilOp's weights are the correlation order: the stencil flipped on both axes
    op = StencilOp((4, 6), st, form="heat", boundary=boundary)
    assert np.array_equal(np.array(op.weights).reshape(3, 3), sr.correlation_weights(st))


@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7)])
def test_transpose_rule_is_the_transposed_matrix(shape, form, boundary):
    ny, nx = shape
    rng = np.random.default_rng(ny * 10 + nx)
    st = rng.standard_normal((3, 3))
    coef = rng.uniform(0.5, 1.5, shape)
    A = sr.dense_matrix(form, st, boundary, coef, ny, nx)
    x = rng.standard_normal(shape if form == "heat" else (2, ny, nx))
    got = sr.transpose_apply(form, st, boundary, coef, x).reshape(-1)
    want = A.T @ x.reshape(-1)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    # the matrix assembled from S and the field (what the GPU tests use at the larger grids) is the column-by-column one
    B, Babs = sr.cached_matrices(form, st, boundary, coef, ny, nx)
    assert np.array_equal(B, A) and np.array_equal(Babs, sr.abs_matrix(form, st, boundary, coef, ny, nx))
    # and the forward matrix is the restated apply (column by column)
    assert np.allclose(A @ x.reshape(-1), sr.apply(form, st, boundary, coef, x).reshape(-1), rtol=1e-13, atol=1e-13)


def _desc(ny=4, nx=6, form=_lib.STENCIL_WAVE, boundary=_lib.BOUNDARY_NEUMANN, n=None, nrows=0, dtype=_lib.MFX_F64):
    desc = _lib.Operator()
    desc.kind, desc.dtype = _lib.OP_STENCIL, dtype
    desc.st_ny, desc.st_nx, desc.st_form, desc.st_boundary = ny, nx, form, boundary
    desc.n = (ny * nx if form == _lib.STENCIL_HEAT else 2 * ny * nx) if n is None else n
    desc.val = 64  # never dereferenced
    desc.st_w = (ctypes.c_double * 9)(0, 1, 0, 1, -2, 1, 0, 1, 0)
    desc.nrows = nrows
    return desc


def test_refusals_come_before_any_launch():
    lib = _lib.get()
    fake = ctypes.c_void_p(64)
    big = 1 << 20

    def apply(desc):
        return lib.mfx_op_apply(ctypes.byref(desc), fake, desc.n, fake, desc.n, 1, 0, fake, big, None)

    def vjp(desc, g):
        return lib.mfx_op_vjp_params(ctypes.byref(desc), fake, desc.n, fake, desc.n, 1, ctypes.byref(g), fake, big, None)

    def forward(desc):
        return lib.mfx_arnoldi_forward(ctypes.byref(desc), fake, desc.n, 2, 1, 1, fake, fake, fake, fake, fake, big, None)

    gval = _lib.OpGrads()
    gval.val = 64
    invalid = [_desc(ny=0, n=48), _desc(nx=0, n=48), _desc(ny=-3, n=48), _desc(n=24), _desc(form=_lib.STENCIL_HEAT, n=48), _desc(n=47), _desc(form=3),
               _desc(form=-1), _desc(boundary=2), _desc(boundary=-1)]
    for desc in invalid:
        for call in (apply, lambda d: vjp(d, gval), forward):
            assert call(desc) == -1, (desc.st_ny, desc.st_nx, desc.st_form, desc.st_boundary, desc.n)
            assert "stencil" in lib.mfx_last_error().decode()
    # grads->x belongs to the kernel-Gram operator
    gx = _lib.OpGrads()
    gx.val = gx.x = 64
    assert vjp(_desc(), gx) == -1 and "kernel-Gram" in lib.mfx_last_error().decode()
    # a row block, and more cells than 2^31 - 1: MFX_ERR_UNSUPPORTED
    for call in (apply, lambda d: vjp(d, gval), forward):
        assert call(_desc(nrows=8)) == -2 and "halo" in lib.mfx_last_error().decode()
        assert call(_desc(ny=65536, nx=32768)) == -2 and "2^31" in lib.mfx_last_error().decode()
    # the row-sharded drivers
    whole = _desc(ny=16, nx=16)
    cm = _lib.Comm()
    cm.rank, cm.world, cm.nloc = 0, 1, 512
    cm.allreduce_sum = _lib.ALLREDUCE_T(lambda *a: 0)
    cm.allgather = _lib.ALLGATHER_T(lambda *a: 0)
    assert lib.mfx_arnoldi_forward_sharded(ctypes.byref(whole), ctypes.byref(cm), fake, 512, 2, 1, 1, fake, fake, fake, fake, fake,
                                           fake, big, None) == -2
    assert "halo" in lib.mfx_last_error().decode()
    assert lib.mfx_lanczos_forward_sharded(ctypes.byref(whole), ctypes.byref(cm), fake, 512, 2, 1, fake, fake, fake, fake, fake, big,
                                           None) == -2
    assert lib.mfx_pcg_solve_sharded(ctypes.byref(whole), ctypes.byref(cm), fake, 512, 512, 1, None, 0, None, None, 3, 0, 0.0, 0.0, 0,
                                     fake, fake, None, fake, big, None) == -2
    assert "halo" in lib.mfx_last_error().decode()
    # the element access of the partial Cholesky keeps refusing the kind
    assert lib.mfx_partial_cholesky(ctypes.byref(whole), 2, 0, 0, fake, fake, fake, fake, big, None) == -2
    # no field gradient asked for: MFX_OK, nothing launched; the operator scratch is the non-Gram 256 bytes
    assert vjp(_desc(), _lib.OpGrads()) == 0
    small = int(lib.mfx_workspace_bytes(ctypes.byref(_desc()), 48, 1, 1))
    dense = _lib.Operator()
    dense.kind, dense.dtype, dense.n = _lib.OP_DENSE, _lib.MFX_F64, 48
    assert small == int(lib.mfx_workspace_bytes(ctypes.byref(dense), 48, 1, 1))


def test_python_layer_refusals_and_shapes():
    st = pde_util.stencil_laplacian(0.5)
    with pytest.raises(NotImplementedError, match="halo exchange"):
        RowShardedOp(StencilOp(8, st), comm=None)
    for bad in (dict(form="waves"), dict(boundary="periodic")):
        with pytest.raises(ValueError):
            StencilOp(4, st, **bad)
    with pytest.raises(ValueError):
        StencilOp((0, 4), st)
    with pytest.raises(ValueError):
        StencilOp(4, torch.zeros(3, 5))
    op = StencilOp((3, 5), st, form="heat2", boundary="dirichlet")
    assert op.size() == 30 and StencilOp(4, st, form="heat").size() == 16
    coef = torch.ones(3, 5, dtype=torch.float64)
    (flat,) = op.constrain(coef)
    assert flat.shape == (15,) and op.constrain() == ()
    desc = op.descriptor((flat,), torch.float64, 30)
    assert (desc.kind, desc.st_ny, desc.st_nx, desc.st_form, desc.st_boundary, desc.val) == (4, 3, 5, 1, 0, flat.data_ptr())
    assert op.descriptor((), torch.float64, 30).val is None
    with pytest.raises(TypeError, match="dtype"):
        op.descriptor((flat.float(),), torch.float64, 30)
    with pytest.raises(ValueError, match="field"):
        op.descriptor((torch.ones(14, dtype=torch.float64),), torch.float64, 30)
    s, g = op.new_grads(flat)
    assert s.val == g[0].data_ptr() and g[0].shape == (15,) and op.new_grads()[1] == ()
    # the vector fields of pde_util carry the bound operator on flattened states where the grid is known
    par, params = pde_util.pde_wave_anisotropic(coef, st, constrain=lambda s: s**2, boundary=pde_util.boundary_neumann())
    assert params["scale"].shape == (3, 5)
    rhs = par(scale=coef)
    assert rhs.flat.op.form == "wave" and rhs.flat.op.boundary == "neumann" and rhs.flat.op.n == 30
    par, params = pde_util.pde_heat(0.3, st, boundary=pde_util.boundary_dirichlet(), shape=(3, 5))
    assert params == {} and np.allclose(par().flat.op.weights, 0.3 * np.array(op.weights))
    with pytest.raises(TypeError, match="boundary"):
        pde_util.pde_heat(0.3, st, boundary=lambda x: x)[0]()
