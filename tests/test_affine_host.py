"""CPU-side checks of the affine operator (MFX_OP_AFFINE, operators.AffineOp; no GPU): the two identities the bordered form rests
on, in the NumPy restatement (tests/_affine_restatement.py); the kind's refusals through the C-ABI before any launch (fake
pointers, a huge ws_bytes, the pattern of tests/test_operator_kinds_host.py); and what AffineOp refuses in Python."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _affine_restatement as ar
from matfree_extensions import _lib
from matfree_extensions.operators import AffineOp, CallbackOp, DenseOp, PreconditionedOp, RbfGramOp, RowShardedOp, StencilOp
from matfree_extensions.util import pde_util, rk_tableaux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)  # never dereferenced
BIG = 1 << 40
M = 3  # unknowns of the inner operator


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", rk_tableaux.NAMES)
def test_runge_kutta_on_the_bordered_system_is_the_scheme_on_the_affine_field(method):
    rng = np.random.default_rng(3)
    m, p = 7, 3
    A, b, y0 = 0.6 * rng.standard_normal((m, m)), rng.standard_normal(m), rng.standard_normal((p, m))
    tab, dts = rk_tableaux.get(method), [0.3, 0.1, 0.25]
    affine = ar.rk_affine(A, b, y0, tab, dts)
    linear = ar.rk_linear(ar.bordered(A, b), ar.lift(y0), tab, dts)
    # two orders of the same few sums: a few hundred roundings of values of O(1) at most (12 stages x 3 steps)
    assert np.abs(linear[:, :m] - affine).max() <= 1e-13 * max(1.0, np.abs(affine).max())
    assert np.array_equal(linear[:, m], np.ones(p))  # the last entry never moves: its row of B is zero


def test_the_exponential_of_the_bordered_matrix_is_the_exponential_integrator():
    rng = np.random.default_rng(4)
    m = 6
    A, b, y0 = 0.5 * rng.standard_normal((m, m)), rng.standard_normal(m), rng.standard_normal(m)
    got = ar.expm(ar.bordered(A, b)) @ ar.lift(y0)
    want = ar.expm(A) @ y0 + ar.phi1_times(A, b)  # t = 1: e^A y0 + phi_1(A) b, phi_1 by its own series
    assert np.abs(got[:m] - want).max() <= 1e-13 * np.abs(want).max()
    assert abs(got[m] - 1.0) <= 1e-15
    # and by quadrature: phi_1(A) b = int_0^1 e^{(1 - s) A} b ds (Gauss-Legendre, 12 nodes: exact far beyond fp64 for |A| ~ 1)
    nodes, weights = np.polynomial.legendre.leggauss(12)
    quad = sum(0.5 * w * ar.expm((1.0 - 0.5 * (s + 1.0)) * A) @ b for s, w in zip(nodes, weights))
    assert np.abs(quad - ar.phi1_times(A, b)).max() <= 1e-13 * np.abs(quad).max()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_mirror_agree_on_the_kind_the_struct_and_the_drift_gradient():
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    assert re.search(r"MFX_OP_AFFINE = 7\b", header) and _lib.OP_AFFINE == 7
    body = header[header.index("typedef struct mfx_affine {") : header.index("} mfx_affine;")]
    assert [f[0] for f in _lib.Affine._fields_] == re.findall(r"\b(\w+);", body) == ["af_inner", "af_b"]
    assert ctypes.sizeof(_lib.Affine) == 2 * ctypes.sizeof(ctypes.c_void_p)
    gbody = header[header.index("typedef struct mfx_op_grads {") : header.index("} mfx_op_grads;")]
    assert [f[0] for f in _lib.OpGrads._fields_] == re.findall(r"\b(\w+);", gbody)
    assert "drift" in [f[0] for f in _lib.OpGrads._fields_]
    assert re.search(r"#define MFX_VERSION 201\b", header) and _lib.get().mfx_version() == 201


def _dense(n=M):
    d = _lib.Operator()
    d.kind, d.dtype, d.n, d.dense_a, d.lda = _lib.OP_DENSE, _lib.MFX_F64, n, 64, n
    return d


def _affine(inner, n=M + 1, b=64):
    af = _lib.Affine()
    af.af_inner, af.af_b = ctypes.addressof(inner), b
    d = _lib.Operator()
    d.kind, d.dtype, d.n, d.ctx = _lib.OP_AFFINE, _lib.MFX_F64, n, ctypes.addressof(af)
    d._keep = (af, inner)
    return d


def _refusals():
    """(label, descriptor, code, text)"""
    yield "null ctx", _affine_null_ctx(), -1, "ctx (the mfx_affine) is NULL"
    yield "null b", _affine(_dense(), b=None), -1, "af_b (the drift) is NULL"
    cb = _lib.Operator()
    cb.kind, cb.dtype, cb.n, cb.callback = _lib.OP_CALLBACK, _lib.MFX_F64, M, _lib.CALLBACK_T(lambda *a: 0)
    yield "inner callback", _affine(cb), -1, "neither preconditioned nor affine itself (kind 3)"
    pc = _dense()
    pc.kind = _lib.OP_PRECOND
    yield "inner precond", _affine(pc), -1, "neither preconditioned nor affine itself (kind 6)"
    yield "inner affine", _affine(_affine(_dense()), n=M + 2), -1, "neither preconditioned nor affine itself (kind 7)"
    broken = _dense()
    broken.dense_a = None
    yield "inner fault", _affine(broken), -1, "dense operator without matrix"
    f32 = _dense()
    f32.dtype = _lib.MFX_F32
    yield "inner dtype", _affine(f32), -1, "dtype 1, inner operator 0"
    yield "wrong n", _affine(_dense(), n=M), -1, "n = 3, but the border of an inner operator of 3 unknowns has 4"
    yield "wrong n", _affine(_dense(), n=M + 2), -1, "n = 5, but the border of an inner operator of 3 unknowns has 4"
    rows = _affine(_dense())
    rows.row0, rows.nrows = 0, 2
    yield "row block", rows, -2, "no row block (nrows > 0): the border row and column belong to no shard"


def _affine_null_ctx():
    d = _lib.Operator()
    d.kind, d.dtype, d.n = _lib.OP_AFFINE, _lib.MFX_F64, M + 1
    return d


def test_the_kind_refuses_before_any_launch_at_apply_and_at_the_drivers():
    lib = _lib.get()
    F, ref = FAKE, ctypes.byref
    grads = _lib.OpGrads()
    grads.drift = 64
    tab = rk_tableaux.struct(rk_tableaux.get("rk4"))
    dts = (ctypes.c_double * 2)(0.5, 0.5)
    seen = 0
    for label, d, code, text in _refusals():
        n = d.n
        calls = {
            "mfx_op_apply": lambda: lib.mfx_op_apply(ref(d), F, n, F, n, 1, 0, F, BIG, None),
            "mfx_op_apply (transposed)": lambda: lib.mfx_op_apply(ref(d), F, n, F, n, 1, 1, F, BIG, None),
            "mfx_op_vjp_params": lambda: lib.mfx_op_vjp_params(ref(d), F, n, F, n, 1, ref(grads), F, BIG, None),
            "mfx_arnoldi_forward": lambda: lib.mfx_arnoldi_forward(ref(d), F, n, 2, 1, 1, F, F, F, F, F, BIG, None),
            "mfx_rk_solve": lambda: lib.mfx_rk_solve(ref(d), ref(tab), dts, 2, F, n, n, 1, F, n, None, 0, F, BIG, None),
            "mfx_rk_adjoint": lambda: lib.mfx_rk_adjoint(ref(d), ref(tab), dts, 2, F, n, 1, F, n, F, n, ref(grads), 0, F, BIG, None),
        }
        for name, call in calls.items():
            got = call()
            assert got == code and text in lib.mfx_last_error().decode(), (label, name, got, lib.mfx_last_error().decode())
            seen += 1
    assert seen == 10 * 6


def test_the_drift_gradient_belongs_to_the_affine_kind_and_row_sharding_is_refused():
    lib = _lib.get()
    F, ref = FAKE, ctypes.byref
    grads = _lib.OpGrads()
    grads.drift = 64
    d = _dense(64)
    assert lib.mfx_op_vjp_params(ref(d), F, 64, F, 64, 1, ref(grads), F, BIG, None) == -1
    assert "the drift gradient (grads->drift) needs an affine operator" in lib.mfx_last_error().decode()
    # the input gradient of a kernel-Gram inner operator is not swept
    gram = _lib.Operator()
    gram.kind, gram.dtype, gram.n, gram.d, gram.kernel_fn = _lib.OP_RBF, _lib.MFX_F64, M, 2, _lib.KERNEL_RBF
    gram.x = gram.lengthscale = gram.outputscale = gram.noise = 64
    gx = _lib.OpGrads()
    gx.x = 64
    a = _affine(gram)
    assert lib.mfx_op_vjp_params(ref(a), F, M + 1, F, M + 1, 1, ref(gx), F, BIG, None) == -2
    assert "grads->x" in lib.mfx_last_error().decode()
    # a preconditioned operator does not wrap an affine one: its sweep would meet the drift gradient under the wrong kind
    pc = _lib.Precond()
    inner = _affine(_dense())
    pc.pc_inner, pc.pc_lt, pc.pc_mid, pc.pc_scale, pc.pc_rank = ctypes.addressof(inner), 64, 64, 64, 1
    outer = _lib.Operator()
    outer.kind, outer.dtype, outer.n, outer.ctx = _lib.OP_PRECOND, _lib.MFX_F64, M + 1, ctypes.addressof(pc)
    for call in (lambda: lib.mfx_op_apply(ref(outer), F, M + 1, F, M + 1, 1, 0, F, BIG, None),
                 lambda: lib.mfx_op_vjp_params(ref(outer), F, M + 1, F, M + 1, 1, ref(_lib.OpGrads()), F, BIG, None)):
        assert call() == -1 and "the inner operator must not be affine" in lib.mfx_last_error().decode(), lib.mfx_last_error().decode()
    # more vectors than a grid has rows
    a = _affine(_dense())
    assert lib.mfx_op_apply(ref(a), F, M + 1, F, M + 1, 65536, 0, F, BIG, None) == -2
    # the row-sharded drivers refuse the kind with its own text
    cm = _lib.Comm()
    cm.rank, cm.world, cm.nloc = 0, 1, 64
    cm.allreduce_sum, cm.allgather = _lib.ALLREDUCE_T(lambda *a: 0), _lib.ALLGATHER_T(lambda *a: 0)
    a = _affine(_dense(63), n=64)
    assert lib.mfx_lanczos_forward_sharded(ref(a), ref(cm), F, 64, 2, 1, F, F, F, F, F, BIG, None) == -2
    assert "row sharding an affine operator is not implemented" in lib.mfx_last_error().decode()
    assert lib.mfx_arnoldi_forward_sharded(ref(a), ref(cm), F, 64, 2, 1, 1, F, F, F, F, F, F, BIG, None) == -2
    assert "row sharding an affine operator is not implemented" in lib.mfx_last_error().decode()


def test_workspace_is_the_inner_operators_plus_the_partial_sums():
    lib = _lib.get()
    for m, p, parts in ((M, 1, 0), (4095, 3, 0), (4096, 3, 2), (3 * 4096 + 5, 2, 4)):  # fp64: a 16-byte pack holds 2 entries
        inner = _dense(m)
        # (the same vector length in both queries: the drivers' own share of the workspace is then the same)
        want = int(lib.mfx_workspace_bytes(ctypes.byref(inner), m + 1, 1, p)) + (p * parts * 8 + 255) // 256 * 256
        a = _affine(inner, n=m + 1)
        assert int(lib.mfx_workspace_bytes(ctypes.byref(a), m + 1, 1, p)) == want, (m, p)


# ---- Python ---------------------------------------------------------------------------------------------------------------------
def test_affine_op_refuses_what_it_cannot_wrap():
    with pytest.raises(TypeError, match="native operator"):
        AffineOp(CallbackOp(lambda v: v))
    with pytest.raises(TypeError, match="affine itself"):
        AffineOp(AffineOp(DenseOp()))
    with pytest.raises(NotImplementedError, match="row sharding an AffineOp"):
        RowShardedOp(AffineOp(DenseOp()), comm=None)
    with pytest.raises(TypeError, match="does not take an AffineOp"):
        PreconditionedOp(AffineOp(DenseOp()), None, None)
    X = torch.zeros((4, 2), requires_grad=True)
    with pytest.raises(NotImplementedError, match="kernel inputs X"):
        AffineOp(RbfGramOp(X))
    with pytest.raises(TypeError, match="AffineOp"):
        pde_util.solver_rk(0.0, 1.0, lambda v: v, num_steps=2, method="rk4")


def test_affine_op_parameters_size_lift_and_drop():
    op = AffineOp(DenseOp())
    A, b = torch.eye(3, dtype=torch.float64), torch.arange(3, dtype=torch.float64).reshape(3, 1)
    cp = op.constrain(A, b)
    assert len(cp) == 2 and cp[1].shape == (3,) and op.size(*cp) == 4
    st = AffineOp(StencilOp((2, 3), pde_util.stencil_laplacian(1.0), form="heat", boundary="neumann"))
    assert st.size(*st.constrain(torch.zeros(2, 3))) == 7
    y = torch.arange(6, dtype=torch.float64).reshape(2, 3).requires_grad_(True)
    z = AffineOp.lift(y)
    assert z.shape == (2, 4) and torch.equal(z[:, 3], torch.ones(2, dtype=torch.float64)) and torch.equal(AffineOp.drop(z), y)
    (g,) = torch.autograd.grad(AffineOp.drop(AffineOp.lift(y)).sum(), y)
    assert torch.equal(g, torch.ones_like(y))
    with pytest.raises(ValueError, match="a drift of 2 values"):
        op.descriptor(op.constrain(A.cuda() if torch.cuda.is_available() else A, b[:2]), torch.float64, 4)


def test_pde_heat_affine_has_a_flat_form():
    drift = torch.zeros((5, 7), dtype=torch.float64)
    par, init = pde_util.pde_heat_affine(0.1, drift, pde_util.stencil_laplacian(1.0), boundary=pde_util.boundary_dirichlet())
    assert init["drift"].shape == (5, 7)
    rhs = par(drift=drift)
    assert isinstance(rhs.flat.op, AffineOp) and isinstance(rhs.flat.op.op, StencilOp)
    assert (rhs.flat.op.op.ny, rhs.flat.op.op.nx, rhs.flat.op.op.form) == (5, 7, "heat")
    assert len(rhs.flat.params) == 1 and rhs.flat.params[0].shape == (35,)
    assert "AffineOp" in pde_util.__doc__


def test_host_refusals_of_the_kind_under_the_sanitizers():
    """`make asan` builds the host code of libmfx under AddressSanitizer + UndefinedBehaviorSanitizer and, with the same flags,
    tests/cabi/cabi_affine_checks.cpp: an affine descriptor around a dense 3 x 3 operator, every fault of it refused through the
    C-ABI before any launch.  A stand-alone program, run here without a GPU."""
    csrc = os.path.join(ROOT, "experiments-lanczos-adjoints_amd", "csrc")
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not (shutil.which("make") and os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists(clang)):
        pytest.skip("needs make, hipcc and the ROCm clang")
    rt = subprocess.run([clang, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("the sanitizer runtime is not installed")
    build = subprocess.run(["make", "-C", csrc, "asan", "-j4"], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
    chk = subprocess.run([os.path.join(csrc, "asan", "cabi_affine_checks")], capture_output=True, text=True, timeout=300)
    assert chk.returncode == 0 and "cabi_affine_checks ok" in chk.stdout, chk.stdout[-2000:] + chk.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in chk.stderr and "runtime error:" not in chk.stderr, chk.stderr[-3000:]
