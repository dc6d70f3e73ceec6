"""The matrix-free 3x3 stencil operator on the GPU against the NumPy restatement (tests/_stencil_restatement.py).

Tile of the shipped kernels (csrc/mfx_stencil.hip): a workgroup covers kStY = 16 rows x kStX = 64 columns.  Grids: the small ones
of the host test, 16 x 16, 17 x 65 (one cell more than a workgroup on each axis) and 19 x 70 (four workgroups, the last one
ragged on both axes).

Bounds.  eps = machine epsilon of the dtype under test.  A result is a sum of at most nine products w coef x and one scaling, so
|y - y_ref| <= 16 eps (|A| |x|) elementwise whatever the order of the sum, where |A| |x| is the sum of the absolute values of
those products: |A| is the operator of |w| and |coef| (_stencil_restatement.abs_matrix).  It equals the entrywise |A| of the dense
matrix except where the padding rule folds weights of opposite sign onto one cell (a Neumann edge); there the dense entry is their
sum, which no evaluation by products can resolve below eps times the products themselves.  The field gradient sums `batch` such
terms: (batch + 12) eps sum_b |L_b| o (|S| |R_b|)."""

import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import torch

import _stencil_restatement as sr
from oracle import slq_oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, arnoldi, lanczos
    from matfree_extensions.operators import StencilOp
    from matfree_extensions.util import pde_util

DEV = torch.device("cuda:0")
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (16, 16), (17, 65), (19, 70)]
DTYPES = [torch.float32, torch.float64]
PS = (1, 3, 5)


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def _case(shape, form, boundary, seed=0):
    """stencil (nine random weights), field and the two restated matrices of a case, in the precision-independent fp64"""
    ny, nx = shape
    rng = np.random.default_rng(1000 * ny + 10 * nx + seed)
    st = rng.standard_normal((3, 3))
    coef = rng.uniform(0.5, 1.5, shape)
    A, Aabs = sr.cached_matrices(form, st, boundary, coef, ny, nx)
    return st, coef, A, Aabs


def _rounded(x, dtype):
    """the fp64 value of x after rounding to dtype: the inputs the device really sees"""
    return N(T(x, dtype))


def _raw_apply(op, coef, X, transpose, ldx=None, ldy=None, out=None):
    """mfx_op_apply through ctypes with explicit leading dimensions"""
    lib = _lib.get()
    p, n = X.shape[0], op.n
    cp = op.constrain(coef) if coef is not None else ()
    desc = op.descriptor(cp, X.dtype, n)
    ws = _lib.workspace(desc, n, 1, p, DEV)
    ldx, ldy = ldx or X.stride(0), ldy or n
    Y = torch.empty((p, ldy), dtype=X.dtype, device=DEV) if out is None else out
    _lib.check(lib.mfx_op_apply(C.byref(desc), _lib.ptr(X), ldx, _lib.ptr(Y), ldy, p, int(transpose), _lib.ptr(ws), ws.numel(),
                                _lib.stream_ptr(DEV)))
    return Y


def _raw_grad(op, coef, L, R, g):
    lib = _lib.get()
    desc = op.descriptor(op.constrain(coef), L.dtype, op.n)
    st = _lib.OpGrads()
    st.val = None if g is None else g.data_ptr()
    ws = _lib.workspace(desc, op.n, 1, L.shape[0], DEV)
    return lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), L.stride(0), _lib.ptr(R), R.stride(0), L.shape[0], C.byref(st),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))


@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_and_transpose_apply_against_the_restated_matrix(shape, form, boundary):
    st, coef, A, Aabs = _case(shape, form, boundary)
    n = A.shape[0]
    rng = np.random.default_rng(7)
    for dtype in DTYPES:
        op = StencilOp(shape, st, form=form, boundary=boundary)
        cf = T(coef, dtype)
        # the device sees the weights and the field rounded to dtype: restate with those (the bound is about the arithmetic)
        Ad, Aabsd = (A, Aabs) if dtype == torch.float64 else sr.cached_matrices(form, _rounded(st, dtype), boundary,
                                                                                  _rounded(coef, dtype), *shape)
        for p in PS:
            X = T(rng.standard_normal((p, n)), dtype)
            Xn = N(X)
            for transpose, M, Mabs in ((False, Ad, Aabsd), (True, Ad.T, Aabsd.T)):
                Y = op(X, cf) if not transpose else _raw_apply(op, cf, X, True)
                err = np.abs(N(Y) - Xn @ M.T)
                bound = 16 * eps_of(dtype) * (np.abs(Xn) @ Mabs.T)
                assert (err <= bound).all(), (dtype, p, transpose, float((err / np.maximum(bound, 1e-300)).max()))
    # without a field: all ones
    op = StencilOp(shape, st, form=form, boundary=boundary)
    A1, A1abs = sr.cached_matrices(form, st, boundary, None, *shape)
    X = T(rng.standard_normal((2, n)))
    assert (np.abs(N(op(X)) - N(X) @ A1.T) <= 16 * eps_of(torch.float64) * (np.abs(N(X)) @ A1abs.T)).all()


def test_apply_with_leading_dimensions_leaves_the_gap_alone():
    shape, form, boundary = (17, 65), "wave", "neumann"
    st, coef, A, Aabs = _case(shape, form, boundary)
    n, p, gap = A.shape[0], 3, 37
    rng = np.random.default_rng(8)
    for transpose in (False, True):
        Xp = torch.full((p, n + gap), float("nan"), dtype=torch.float64, device=DEV)
        Xp[:, :n] = T(rng.standard_normal((p, n)))
        Yp = torch.full((p, n + 2 * gap), -777.0, dtype=torch.float64, device=DEV)
        _raw_apply(StencilOp(shape, st, form=form, boundary=boundary), T(coef), Xp, transpose, ldx=n + gap, ldy=n + 2 * gap, out=Yp)
        assert bool((Yp[:, n:] == -777.0).all())
        M, Mabs = (A.T, Aabs.T) if transpose else (A, Aabs)
        Xn = N(Xp[:, :n])
        assert (np.abs(N(Yp[:, :n]) - Xn @ M.T) <= 16 * eps_of(torch.float64) * (np.abs(Xn) @ Mabs.T)).all()


@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_field_gradient_is_added_once(shape, form, boundary):
    st, coef, A, _ = _case(shape, form, boundary)
    ny, nx = shape
    n = A.shape[0]
    rng = np.random.default_rng(9)
    for dtype in DTYPES:
        op = StencilOp(shape, st, form=form, boundary=boundary)
        std = st if dtype == torch.float64 else _rounded(st, dtype)
        for batch in (1, 4, 33):
            L, R = T(rng.standard_normal((batch, n)), dtype), T(rng.standard_normal((batch, n)), dtype)
            g0 = T(rng.standard_normal(ny * nx), dtype)
            g = g0.clone()
            assert _raw_grad(op, T(coef, dtype), L, R, g) == 0
            want = N(g0).reshape(shape) + sr.field_gradient(form, std, boundary, N(L), N(R), ny, nx)
            # + one rounding of the final add onto the pre-filled value
            bound = (batch + 12) * eps_of(dtype) * sr.field_gradient_bound(form, std, boundary, N(L), N(R), ny, nx) \
                + eps_of(dtype) * np.abs(want)
            err = np.abs(N(g).reshape(shape) - want)
            assert (err <= bound).all(), (dtype, batch, float((err / np.maximum(bound, 1e-300)).max()))
    # no gradient asked for: MFX_OK, and nothing is written anywhere
    assert _raw_grad(op, T(coef, dtype), L, R, None) == 0


@pytest.mark.parametrize("form", sr.FORMS)
def test_autograd_round_trip(form):
    shape, boundary = (3, 7), "neumann"
    st, coef, A, Aabs = _case(shape, form, boundary)
    ny, nx = shape
    n = A.shape[0]
    rng = np.random.default_rng(10)
    op = StencilOp(shape, st, form=form, boundary=boundary)
    for p in (None, 3):
        v = T(rng.standard_normal(n if p is None else (p, n)), grad=True)
        cf = T(coef, grad=True)  # (ny, nx): the gradient comes back in that shape
        w = T(rng.standard_normal(v.shape))
        dv, dc = torch.autograd.grad((w * op(v, cf)).sum(), (v, cf))
        W, V = np.atleast_2d(N(w)), np.atleast_2d(N(v))
        assert dc.shape == (ny, nx)
        assert (np.abs(np.atleast_2d(N(dv)) - W @ A) <= 16 * eps_of(torch.float64) * (np.abs(W) @ Aabs)).all()
        want = sr.field_gradient(form, st, boundary, W, V, ny, nx)
        bound = (len(W) + 12) * eps_of(torch.float64) * sr.field_gradient_bound(form, st, boundary, W, V, ny, nx)
        assert (np.abs(N(dc) - want) <= bound).all()


def test_three_kernels_are_bit_reproducible():
    shape, form, boundary = (19, 70), "heat2", "neumann"
    st, coef, A, _ = _case(shape, form, boundary)
    n = A.shape[0]
    rng = np.random.default_rng(11)
    for dtype in DTYPES:
        op, cf = StencilOp(shape, st, form=form, boundary=boundary), T(coef, dtype)
        X, L = T(rng.standard_normal((5, n)), dtype), T(rng.standard_normal((33, n)), dtype)
        R = T(rng.standard_normal((33, n)), dtype)
        for transpose in (False, True):
            assert torch.equal(_raw_apply(op, cf, X, transpose), _raw_apply(op, cf, X, transpose))
        g1, g2 = torch.zeros(n // 2, dtype=dtype, device=DEV), torch.zeros(n // 2, dtype=dtype, device=DEV)
        assert _raw_grad(op, cf, L, R, g1) == 0 and _raw_grad(op, cf, L, R, g2) == 0
        assert torch.equal(g1, g2) and bool(g1.abs().sum() > 0)


@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
@pytest.mark.parametrize("res", [8, 16])
def test_same_numbers_as_the_assembled_csr_operator(res, boundary):
    dx = 1.0 / (res - 1)
    rng = np.random.default_rng(res)
    st = pde_util.stencil_laplacian(dx).numpy()
    coef = rng.uniform(0.5, 1.5, (res, res))
    _, Aabs = sr.cached_matrices("wave", st, boundary, coef, res, res)
    csr, values_fn = pde_util.wave_operator(res, dx, boundary=boundary, device=DEV)
    op = StencilOp(res, st, form="wave", boundary=boundary)
    n, eps = op.n, eps_of(torch.float64)
    X = T(rng.standard_normal((3, n)))
    W = T(rng.standard_normal((3, n)))
    c1, c2 = T(coef, grad=True), T(coef, grad=True)
    x1, x2 = X.clone().requires_grad_(True), X.clone().requires_grad_(True)
    vals = values_fn(c2)
    y1, y2 = op(x1, c1), csr(x2, vals)
    # both are within 16 eps |A| |x| of the exact product: of each other within twice that
    assert (np.abs(N(y1) - N(y2)) <= 32 * eps * (np.abs(N(X)) @ Aabs.T)).all()
    g1 = torch.autograd.grad((W * y1).sum(), (x1, c1))
    g2 = torch.autograd.grad((W * y2).sum(), (x2, c2, vals))
    assert (np.abs(N(g1[0]) - N(g2[0])) <= 32 * eps * (np.abs(N(W)) @ Aabs)).all()
    bound = 2 * (3 + 12) * eps * sr.field_gradient_bound("wave", st, boundary, N(W), N(X), res, res)
    # the CSR sweep's gradient of the stored values, carried to the field by values_fn's rule (weight x value gradient, summed over
    # the entries of a cell's row) in exact-order fp64 on the host: the bounds above
    m = res * res
    crow = csr.crow.cpu().numpy()
    wd = N(g2[2]) * N(values_fn(torch.ones(m, dtype=torch.float64, device=DEV)))
    host = np.array([wd[crow[m + r] : crow[m + r + 1]].sum() for r in range(m)]).reshape(res, res)
    assert (np.abs(N(g1[1]) - host) <= bound).all()
    # values_fn's own backward takes differences of ONE running sum over all 6 res^2 entries (a parallel scan: at most
    # ceil(log2 N) + 1 additions per prefix), so its error scales with the running total, not with a cell's own terms: that error
    # of the reference route is added to the bound
    scan = 2 * (np.ceil(np.log2(wd.size)) + 1) * eps * np.abs(wd[crow[m] :]).sum()
    assert (np.abs(N(g1[1]) - N(g2[1]).reshape(res, res)) <= bound + scan).all()


# the tolerances of tests/test_gpu_next_tier.py:119 for the CSR wave operator through expm_arnoldi in fp64 (rtol 1e-8, atol 1e-8 of
# the largest entry); that file has no shallower case for the wave system, so the k = 6 comparison below uses the same figures
def _close(got, want):
    return np.allclose(got, want, rtol=1e-8, atol=1e-8 * max(np.abs(want).max(), 1e-300))


def _driver_problem():
    ny, nx, k, p = 6, 7, 6, 2
    st = pde_util.stencil_advection_diffusion(0.25).numpy()
    rng = np.random.default_rng(12)
    coef = rng.uniform(0.5, 1.5, (ny, nx))
    V = rng.standard_normal((p, 2 * ny * nx))
    cot = dict(dQ=rng.standard_normal((p, 2 * ny * nx, k)), dH=rng.standard_normal((p, k, k)), dr=rng.standard_normal((p, 2 * ny * nx)),
               dc=rng.standard_normal(p))
    return ny, nx, k, p, st, coef, V, cot


@pytest.mark.parametrize("bound", [False, True], ids=["op", "op.bind"])
def test_arnoldi_forward_and_adjoint_against_the_oracle(bound):
    ny, nx, k, p, st, coef, V, cot = _driver_problem()
    A = sr.dense_matrix("wave", st, "neumann", coef, ny, nx)
    op = StencilOp((ny, nx), st, form="wave", boundary="neumann")
    v, cf = T(V, grad=True), T(coef, grad=True)
    if bound:
        Q, H, r, c = arnoldi.hessenberg(op.bind(cf), k, reortho="full")(v)
    else:
        Q, H, r, c = arnoldi.hessenberg(op, k, reortho="full")(v, cf)
    loss = (Q * T(cot["dQ"])).sum() + (H * T(cot["dH"])).sum() + (r * T(cot["dr"])).sum() + (c * T(cot["dc"])).sum()
    dv, dcoef = torch.autograd.grad(loss, (v, cf))
    want_dcoef = np.zeros((ny, nx))
    for b in range(p):
        Qo, Ho, ro, co = orc.arnoldi_forward(orc.DenseOp(), k, V[b], A, reortho="full")
        for got, want in ((Q[b], Qo), (H[b], Ho), (r[b], ro), (c[b], co)):
            assert _close(N(got), want)
        dvo, (dA,) = orc.arnoldi_adjoint(orc.DenseOp(), (A,), Q=Qo, H=Ho, r=ro, c=co, dQ=cot["dQ"][b], dH=cot["dH"][b], dr=cot["dr"][b],
                                         dc=cot["dc"][b], reortho="full")
        assert _close(N(dv[b]), dvo)
        want_dcoef += sr.contract_dense_gradient("wave", st, "neumann", dA, ny, nx)
    assert _close(N(dcoef), want_dcoef)


def test_solver_expm_takes_the_bound_operator_of_the_wave_field():
    ny, nx, k, p, st, coef, V, _ = _driver_problem()
    rng = np.random.default_rng(13)
    raw = np.sqrt(coef)
    t1 = 0.01
    y0, w = V[0].reshape(2, ny, nx), rng.standard_normal((2, ny, nx))
    sc = T(raw, grad=True)
    par, _ = pde_util.pde_wave_anisotropic(sc, torch.tensor(st), constrain=lambda s: s**2, boundary=pde_util.boundary_neumann())
    rhs = par(scale=sc)
    # the vector field on (2, ny, nx) states is the reference's
    assert np.allclose(N(rhs(T(y0))), sr.apply("wave", st, "neumann", raw**2, y0), rtol=1e-12, atol=1e-12)
    y1, info = pde_util.solver_expm(0.0, t1, rhs.flat, pde_util.expm_arnoldi(k))(T(y0))
    assert info["num_matvecs"] == k and y1.shape == (2, ny, nx)

    def oracle(raw_):
        A = sr.dense_matrix("wave", st, "neumann", raw_**2, ny, nx)
        Q, H, _r, c = orc.arnoldi_forward(orc.DenseOp(), k, y0.reshape(-1), A, reortho="full")
        return Q @ scipy.linalg.expm(t1 * H)[:, 0] / c

    assert _close(N(y1).reshape(-1), oracle(raw))
    (g,) = torch.autograd.grad((y1 * T(w)).sum(), sc)
    d = rng.standard_normal((ny, nx))
    h = 1e-6
    fd = (w.reshape(-1) @ oracle(raw + h * d) - w.reshape(-1) @ oracle(raw - h * d)) / (2 * h)
    assert abs((N(g) * d).sum() - fd) <= 1e-5 * max(1.0, abs(fd))  # tests/test_gpu_next_tier.py:132


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 5e-6), (torch.float32, 2e-5)])
def test_pde_wave_reference_targets_through_the_stencil_operator(dtype, tol):
    """tests/golden/pde_wave_16x16.npz holds reference-produced inputs and targets; the bounds are those of
    tests/test_gpu_configs.py::test_pde_wave_reference_targets_through_expm_arnoldi."""
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pde_wave_16x16.npz"))
    op = StencilOp(16, pde_util.stencil_laplacian(1.0 / 15.0), form="wave", boundary="neumann")
    coef = torch.tensor(g["parameter"].astype(np.float64) ** 2, dtype=dtype, device=DEV)
    expm = pde_util.expm_arnoldi(12)
    for y0, y1 in zip(g["inputs"], g["targets"]):
        out, info = expm(op, 1.0, torch.tensor(y0.reshape(-1), dtype=dtype, device=DEV), coef)
        assert info["num_matvecs"] == 12
        err = np.abs(N(out).reshape(y1.shape) - y1.astype(np.float64)).max()
        assert err <= tol * np.abs(y1).max(), err


def test_symmetric_heat_system_lanczos_and_arnoldi_agree():
    """Dirichlet heat with a constant field is symmetric: expm_lanczos(12) and expm_arnoldi(12) span the same Krylov space.  1e-10 of
    the largest entry: the fp64 value tolerance of tests/test_gpu_funm.py (VALUE_TOL) for expm_lanczos on its own operators."""
    ny, nx = 7, 9
    st = pde_util.stencil_laplacian(0.25).numpy()
    A = sr.dense_matrix("heat", st, "dirichlet", np.full((ny, nx), 0.7), ny, nx)
    assert np.array_equal(A, A.T)
    op = StencilOp((ny, nx), st, form="heat", boundary="dirichlet")
    cf = torch.full((ny, nx), 0.7, dtype=torch.float64, device=DEV)
    y0 = T(np.random.default_rng(14).standard_normal(ny * nx))
    a, _ = pde_util.expm_arnoldi(12)(op, 0.01, y0, cf)
    b, _ = pde_util.expm_lanczos(12)(op, 0.01, y0, cf)
    assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max())
    # and through lanczos.tridiag / funm_spd directly, bound
    c = lanczos.funm_spd(lambda lam: torch.exp(0.01 * lam), 12, op.bind(cf))(y0)
    assert float((c - b).abs().max()) <= 1e-10 * float(b.abs().max())
