"""The affine operator on the GPU (MFX_OP_AFFINE, csrc/mfx_affine.hip, operators.AffineOp) against the fp64 dense restatement
(tests/_affine_restatement.py): the bordered apply, transposed apply and drift gradient; then solver_rk and solver_expm on affine
fields with their gradients.

Sizes.  The border kernels move 16-byte packs (4 floats, 2 doubles), a wave 64 of them, a workgroup SPAN = 4096 entries; the inner
sizes put the border entry on and next to each of these boundaries, and SPAN + 1 is the one size at which k_affine_dot takes its
second stage (two workgroups per probe).  The bordered length m + 1 is odd for even m, so with p = 3 the middle probe starts
misaligned; one case pads the leading dimensions on top.

Bounds.  Operator level, elementwise, the tolerances the inner operators' own GPU tests apply to the same quantity:
  stencil inner   |y - y_ref| <= 16 eps (|B| |x|), the bound of tests/test_gpu_stencil.py for both applies.  It still holds with the
                  border: a bordered row is the stencil's at most nine products and one scaling plus ONE more product and addition,
                  12 roundings of at most eps / 2 each against 16 eps; the border entry of the transposed apply is a sum formed in
                  fp64 and rounded once.
  dense inner     _ragged_csr.apply_bound(m + 1, u, |B| |x|) = 2 (m + 1 + 8) u (|B| |x|), the bound of
                  tests/test_gpu_operator_kernels.py for a row of m + 1 products summed in any order (derived there).
  drift gradient  _ragged_csr.grad_bound(batch, u, sum_b |R_b[m]| |L_b|, prefill): a sum in fp64, rounded to the dtype, added once
                  onto what the buffer holds -- the bound of the dense and CSR gradient tests, and the arithmetic of k_affine_grad_b.
  adjointness     <Y, B X> - <B^T Y, X> = <Y, B X - ref> - <B^T Y - ref^T, X>: each apply within f (|B| |x|) of the restatement gives
                  at most 2 f |Y|^T |B| |X|, f the factor of the apply bound above; the two fp64 sums over n p terms formed on the
                  host add 4 n p 2^-53 of the same quantity.
Solver level: the parity tolerances of tests/test_gpu_rk.py, 1e-10 (fp64) and 1e-4 (fp32) of the largest entry of the restated quantity, with step
sizes as stable as there (dt |A| <= 1: weights of O(1), a field in [0.3, 0.8], t1 - t0 = 0.2)."""

import ctypes as C

import numpy as np
import pytest
import torch

import _affine_restatement as ar
import _ragged_csr as rc
import _rk_restatement as rr
import _stencil_restatement as sr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib
    from matfree_extensions.operators import AffineOp, DenseOp, StencilOp
    from matfree_extensions.util import pde_util, rk_tableaux

DEV = torch.device("cuda:0")
SPAN = 4096  # kAfSpan of csrc/mfx_affine.hip: entries of one vector per workgroup
SECOND_STAGE = SPAN + 1  # the smallest inner size with two workgroups per probe in k_affine_dot
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
DTYPES = [torch.float64, torch.float32]
TOL = {torch.float64: 1e-10, torch.float32: 1e-4}
T1 = 0.2


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def H(t):
    return t.detach().cpu().to(torch.float64)


def rounded(x, dtype):
    """the fp64 value of x after rounding to dtype: what the device really sees"""
    return torch.tensor(np.asarray(x)).to(dtype).to(torch.float64).numpy()


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def close(got, want, dtype, what):
    want = torch.as_tensor(np.asarray(want))
    err, scale = float((H(got).reshape(want.shape) - want).abs().max()), float(want.abs().max())
    print(f"{what}: max error {err:.3e}, largest entry {scale:.3e}, ratio {err / max(scale, 1e-300):.3e}")
    assert err <= TOL[dtype] * scale, (what, dtype, err, scale)


# ---- operator level ---------------------------------------------------------------------------------------------------------------
def _grid_of(m):
    """a grid of m cells with more than one row where m allows it"""
    for ny in (16, 5, 3, 2):
        if m % ny == 0 and m > ny:
            return ny, m // ny
    return 1, m


def _case(inner, m, dtype):
    """(operator, its parameters on the device, dense bordered B, |B|, factor f of the apply bound f (|B| |x|)) with the data rounded
    to dtype.  Nothing is kept between tests: a test leaves no device memory behind."""
    u = rc.unit_roundoff("float64" if dtype == torch.float64 else "float32")
    rng = np.random.default_rng(7 * m + (inner == "dense"))
    b = rounded(rng.standard_normal(m), dtype)
    if inner == "dense":
        A = rounded(rng.standard_normal((m, m)) / np.sqrt(m), dtype)
        op, params, Aabs, factor = AffineOp(DenseOp()), (T(A, dtype),), np.abs(A), float(rc.apply_bound(m + 1, u, 1.0))
    else:
        ny, nx = _grid_of(m)
        st, coef = rounded(rng.standard_normal((3, 3)), dtype), rounded(rng.uniform(0.5, 1.5, (ny, nx)), dtype)
        A, Aabs = sr.cached_matrices("heat", st, "neumann", coef, ny, nx)
        op, params, factor = AffineOp(StencilOp((ny, nx), st, form="heat", boundary="neumann")), (T(coef, dtype),), 16 * eps_of(dtype)
    return op, params + (T(b, dtype),), ar.bordered(A, b), ar.bordered(Aabs, np.abs(b)), factor


def _raw_apply(op, params, X, n, transpose, ldy=None):
    lib = _lib.get()
    p = X.shape[0]
    desc = op.descriptor(op.constrain(*params), X.dtype, n)
    ws = _lib.workspace(desc, n, 1, p, DEV)
    ldy = ldy or n
    Y = torch.full((p, ldy), -777.0, dtype=X.dtype, device=DEV)
    _lib.check(lib.mfx_op_apply(C.byref(desc), _lib.ptr(X), X.stride(0), _lib.ptr(Y), ldy, p, int(transpose), _lib.ptr(ws), ws.numel(),
                                _lib.stream_ptr(DEV)))
    return Y


def _raw_drift_grad(op, params, L, R, n, g):
    lib = _lib.get()
    desc = op.descriptor(op.constrain(*params), L.dtype, n)
    st = _lib.OpGrads()
    st.drift = g.data_ptr()
    ws = _lib.workspace(desc, n, 1, L.shape[0], DEV)
    _lib.check(lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(L), L.stride(0), _lib.ptr(R), R.stride(0), L.shape[0], C.byref(st),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))


def _check_operator(inner, m, dtype, p, pad=0, case=None):
    op, params, B, Babs, factor = case or _case(inner, m, dtype)
    n, u = m + 1, eps_of(dtype) / 2
    rng = np.random.default_rng(100 * m + p)
    Xp = torch.full((p, n + pad), float("nan"), dtype=dtype, device=DEV)
    Yp = torch.full((p, n + pad), float("nan"), dtype=dtype, device=DEV)
    Xp[:, :n], Yp[:, :n] = T(rng.standard_normal((p, n)), dtype), T(rng.standard_normal((p, n)), dtype)
    X, Y = Xp[:, :n], Yp[:, :n]
    Xn, Yn = N(X), N(Y)
    # apply and transposed apply, elementwise; the padding of the outputs stays as it was
    BX = _raw_apply(op, params, Xp if pad else X.contiguous(), n, False, ldy=n + 2 * pad)
    BtY = _raw_apply(op, params, Yp if pad else Y.contiguous(), n, True, ldy=n + 2 * pad)
    assert bool((BX[:, n:] == -777.0).all()) and bool((BtY[:, n:] == -777.0).all())
    for got, ref, bound in ((BX, Xn @ B.T, np.abs(Xn) @ Babs.T), (BtY, Yn @ B, np.abs(Yn) @ Babs)):
        err = np.abs(N(got[:, :n]) - ref)
        assert (err <= factor * bound).all(), (inner, m, dtype, p, float((err / np.maximum(factor * bound, 1e-300)).max()))
    assert bool((BX[:, m] == 0).all())  # the border row is zero, exactly
    # adjointness <Y, B X> = <B^T Y, X> (the bound: module docstring)
    lhs, rhs = float((Yn * N(BX[:, :n])).sum()), float((N(BtY[:, :n]) * Xn).sum())
    assert abs(lhs - rhs) <= (2 * factor + 4 * n * p * 2.0**-53) * float((np.abs(Yn) * (np.abs(Xn) @ Babs.T)).sum())
    # the drift gradient is added once onto what the buffer holds
    for batch in (p, 5):
        L, R = T(rng.standard_normal((batch, n)), dtype), T(rng.standard_normal((batch, n)), dtype)
        g0 = T(rng.standard_normal(m), dtype)
        g = g0.clone()
        _raw_drift_grad(op, params, L, R, n, g)
        mag = (np.abs(N(R)[:, m:]) * np.abs(N(L)[:, :m])).sum(0)
        want = N(g0) + (N(R)[:, m:] * N(L)[:, :m]).sum(0)
        assert (np.abs(N(g) - want) <= rc.grad_bound(batch, u, mag, N(g0))).all(), (inner, m, dtype, batch)
        # two calls, equal bits
        g2 = g0.clone()
        _raw_drift_grad(op, params, L, R, n, g2)
        assert torch.equal(g, g2)
    assert torch.equal(BtY, _raw_apply(op, params, Yp if pad else Y.contiguous(), n, True, ldy=n + 2 * pad))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("inner", ["dense", "stencil"])
@pytest.mark.parametrize("m", SIZES)
def test_apply_transpose_and_drift_gradient_against_the_dense_bordered_matrix(m, inner, dtype):
    case = _case(inner, m, dtype)  # the restated matrices once for both batch sizes
    for p in (1, 3):
        _check_operator(inner, m, dtype, p, case=case)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_second_reduction_stage_and_padded_leading_dimensions(dtype):
    _check_operator("dense", SECOND_STAGE, dtype, 3)  # two workgroups per probe in all three kernels, partial sums from the workspace
    _check_operator("stencil", 1024, dtype, 3, pad=3)  # ld = 1028 and 1031: every probe starts at another offset of a pack
    _check_operator("dense", 65, dtype, 3, pad=1)


def test_autograd_through_the_operator_reaches_the_inner_parameters_and_the_drift():
    m, dtype = 65, torch.float64
    op, params, B, _, _ = _case("dense", m, dtype)  # (autograd through the operator: the parity tolerance of `close`)
    A, b = (q.detach().clone().requires_grad_(True) for q in params)
    x = T(np.random.default_rng(1).standard_normal((3, m + 1)), grad=True)
    w = T(np.random.default_rng(2).standard_normal((3, m + 1)))
    gx, gA, gb = torch.autograd.grad(op(x, A, b), [x, A, b], w)
    Bt = torch.tensor(B, requires_grad=True)
    xt = H(x).requires_grad_(True)
    rx, rB = torch.autograd.grad(xt @ Bt.T, [xt, Bt], H(w))
    close(gx, rx, dtype, "dx")
    close(gA, rB[:m, :m], dtype, "dA")
    close(gb, rB[:m, m], dtype, "ddrift")


# ---- solver_rk ----------------------------------------------------------------------------------------------------------------------
def _stencil():
    return pde_util.stencil_advection_diffusion(1.0).numpy()


def _affine_field(form, grid, boundary, dtype):
    """-> (solver argument factory, params that need gradients, dense A fp64, b fp64, map from a dense cotangent of A to the field's)"""
    ny, nx = grid
    rng = np.random.default_rng(100 * ny + nx)
    st = _stencil()
    st_dev = rounded(st, dtype)
    m = sr.state_size(form, ny, nx)
    b = rounded(rng.standard_normal(m), dtype)
    if form == "heat":  # pde_heat_affine: the constant c folded into the weights, no coefficient field
        c = 0.7
        drift = T(b.reshape(ny, nx), dtype, grad=True)
        bnd = pde_util.boundary_neumann() if boundary == "neumann" else pde_util.boundary_dirichlet()
        par, _ = pde_util.pde_heat_affine(c, drift.detach(), st, boundary=bnd)
        A = ar.stencil_dense("heat", rounded(c * st, dtype), boundary, None, ny, nx)
        return par(drift=drift).flat, (), (drift,), A, b, None
    coef = rounded(rng.uniform(0.3, 0.8, (ny, nx)), dtype)
    op = AffineOp(StencilOp(grid, st, form=form, boundary=boundary))
    A = ar.stencil_dense(form, st_dev, boundary, coef, ny, nx)
    back = lambda dA: sr.contract_dense_gradient(form, st_dev, boundary, np.asarray(dA), ny, nx)  # noqa: E731
    return op, (T(coef, dtype, grad=True), T(b, dtype, grad=True)), (), A, b, back


def _reference(A, b, y0, w, tab, dts, adjoint):
    """(y1, dy0, dA, db) in fp64 torch.  discrete: autograd through the scheme written on the AFFINE form y' = A y + b.  backsolve:
    the restated continuous-adjoint recursion (tests/_rk_restatement.py) on the bordered matrix, as tests/test_gpu_rk.py does for
    linear fields."""
    m = A.shape[0]
    At, bt, yt = (torch.tensor(v, requires_grad=True) for v in (A, b, y0))
    y1 = rr.solve(lambda Y: Y @ At.T + bt, yt, tab, dts)
    if adjoint == "discrete":
        dy0, dA, db = torch.autograd.grad(y1, [yt, At, bt], torch.tensor(w))
        return y1.detach(), dy0, dA, db
    z1 = torch.tensor(ar.lift(y1.detach().numpy()))
    dz1 = torch.cat([torch.tensor(w), torch.zeros((w.shape[0], 1), dtype=torch.float64)], 1)
    dz0, dB = rr.backsolve(torch.tensor(ar.bordered(A, b)), z1, dz1, tab, dts)
    return y1.detach(), dz0[:, :m], dB[:m, :m], dB[:m, m]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
@pytest.mark.parametrize("form", ["heat", "wave", "heat2"])
@pytest.mark.parametrize("grid", [(1, 1), (5, 7), (16, 16)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_solver_rk_on_affine_fields_against_the_restatement(grid, form, boundary, dtype):
    field, params, closed, A, b, back = _affine_field(form, grid, boundary, dtype)
    m = A.shape[0]
    rng = np.random.default_rng(11)
    y0n, wn = rounded(rng.standard_normal((1, m)), dtype), rounded(rng.standard_normal((1, m)), dtype)
    shape = grid if form == "heat" else (2, *grid)
    for method in ("euler", "rk4", "dopri5"):
        tab = rk_tableaux.get(method)
        for steps in (1, 3):
            dts = [T1 / steps] * steps
            value = ar.rk_affine(A, b, y0n, tab, dts)  # the NumPy loop on the affine form
            for adjoint in ("discrete", "backsolve"):
                ref_y1, ref_dy0, ref_dA, ref_db = _reference(A, b, y0n, wn, tab, dts, adjoint)
                solver = pde_util.solver_rk(0.0, T1, field, num_steps=steps, method=method, adjoint=adjoint)
                y0 = T(y0n.reshape(shape), dtype, grad=True)
                y1, info = solver(y0, *params)
                assert y1.shape == y0.shape and info == {"num_matvecs": steps * tab.order, "num_applies": steps * len(tab.b)}
                grads = torch.autograd.grad(y1, [y0, *params, *closed], T(wn.reshape(shape), dtype))
                what = f"{form} {boundary} {method} x{steps} {adjoint}"
                close(y1, value.reshape(shape), dtype, what + " y1 (NumPy affine loop)")
                close(y1, ref_y1.reshape(shape), dtype, what + " y1")
                close(grads[0], ref_dy0.reshape(shape), dtype, what + " dy0")
                close(grads[-1], ref_db.reshape(grads[-1].shape), dtype, what + " ddrift")
                if back is not None:
                    close(grads[1], back(ref_dA), dtype, what + " dcoef")


def test_dopri5_with_nine_steps_is_one_driver_call_for_every_adjoint_name():
    grid = (16, 16)
    field, _, (drift,), A, b, _ = _affine_field("heat", grid, "neumann", torch.float64)
    rng = np.random.default_rng(12)
    y0n, wn = rng.standard_normal((1, 256)), rng.standard_normal((1, 256))
    tab, dts = rk_tableaux.get("dopri5"), [1.0 / 9] * 9
    for adjoint in ("recursive_checkpoint", "direct", "backsolve"):
        ref = _reference(A, b, y0n, wn, tab, dts, "backsolve" if adjoint == "backsolve" else "discrete")
        y0 = T(y0n.reshape(grid), grad=True)
        y1, _ = pde_util.solver_rk(0, 1, field, num_steps=9, method="dopri5", adjoint=adjoint)(y0)
        dy0, dd = torch.autograd.grad(y1, [y0, drift], T(wn.reshape(grid)))
        close(y1, ref[0].reshape(grid), torch.float64, f"{adjoint} y1")
        close(dy0, ref[1].reshape(grid), torch.float64, f"{adjoint} dy0")
        close(dd, ref[3].reshape(grid), torch.float64, f"{adjoint} ddrift")


def test_solver_euler_and_a_batch_of_states():
    grid = (5, 7)
    field, _, _, A, b, _ = _affine_field("heat", grid, "dirichlet", torch.float64)
    rng = np.random.default_rng(13)
    yb = rng.standard_normal((3, 5, 7))
    ts = np.cumsum([0.0, 0.05, 0.1, 0.05])
    got, info = pde_util.solver_euler(ts, field)(T(yb))
    assert got.shape == (3, 5, 7) and info["num_applies"] == 3
    close(got, ar.rk_affine(A, b, yb.reshape(3, 35), rk_tableaux.get("euler"), np.diff(ts)).reshape(3, 5, 7), torch.float64, "euler batch")
    solver = pde_util.solver_rk(0.0, T1, field, num_steps=3, method="rk4")
    batch, _ = solver(T(yb))
    for i in range(3):  # a batch of three states gives the three single-state results
        single, _ = solver(T(yb[i]))
        assert single.shape == (5, 7)
        close(batch[i], H(single), torch.float64, f"state {i} of the batch")
    with pytest.raises(ValueError, match="does not match"):
        solver(T(np.ones(36)))


# ---- solver_expm ----------------------------------------------------------------------------------------------------------------
def test_solver_expm_with_full_depth_arnoldi_is_the_dense_exponential_of_the_bordered_matrix():
    grid = (4, 4)
    field, _, (drift,), A, b, _ = _affine_field("heat", grid, "neumann", torch.float64)
    rng = np.random.default_rng(14)
    y0n, wn = rng.standard_normal(16), rng.standard_normal(16)
    solve = pde_util.solver_expm(0.0, 0.5, field, expm=pde_util.expm_arnoldi(17))
    y0 = T(y0n.reshape(grid), grad=True)
    y1, info = solve(y0)
    assert y1.shape == (4, 4) and info == {"num_matvecs": 17}
    dy0, dd = torch.autograd.grad(y1, [y0, drift], T(wn.reshape(grid)))
    At, bt, yt = (torch.tensor(v, requires_grad=True) for v in (A, b, y0n))
    Bt = torch.cat([torch.cat([At, bt[:, None]], 1), torch.zeros((1, 17), dtype=torch.float64)], 0)
    ref = (torch.linalg.matrix_exp(0.5 * Bt) @ torch.cat([yt, torch.ones(1, dtype=torch.float64)]))[:16]
    rdy0, rdb = torch.autograd.grad(ref, [yt, bt], torch.tensor(wn))
    close(y1, ref.detach().reshape(grid), torch.float64, "expm y1")
    close(y1, (ar.expm(0.5 * ar.bordered(A, b)) @ ar.lift(y0n))[:16].reshape(grid), torch.float64, "expm y1 (NumPy)")
    close(dy0, rdy0.reshape(grid), torch.float64, "expm dy0")
    close(dd, rdb.reshape(grid), torch.float64, "expm ddrift")
    # a batch of states lifts each state
    yb = rng.standard_normal((3, 4, 4))
    got, _ = solve(T(yb))
    want = (ar.lift(yb.reshape(3, 16)) @ ar.expm(0.5 * ar.bordered(A, b)).T)[:, :16]
    close(got, want.reshape(3, 4, 4), torch.float64, "expm batch")


# ---- what does not change, and the graph replay ---------------------------------------------------------------------------------
def test_an_unbordered_stencil_operator_gives_the_bits_of_the_plain_driver_call():
    grid = (5, 7)
    op = StencilOp(grid, _stencil(), form="wave", boundary="neumann")
    coef = T(np.random.default_rng(15).uniform(0.3, 0.8, grid))
    y0 = T(np.random.default_rng(16).standard_normal((2, 5, 7)))
    tab = rk_tableaux.get("rk4")
    y1, _ = pde_util.solver_rk(0.0, T1, op, num_steps=3, method="rk4")(y0, coef)
    direct, _ = pde_util._rk_forward(op, op.constrain(coef), tab, (T1 / 3,) * 3, y0.reshape(1, -1), False)
    assert y1.shape == y0.shape and torch.equal(y1.reshape(-1), direct.reshape(-1))
    close(y1, rr.solve(torch.tensor(rr.stencil_case("wave", _stencil(), "neumann", N(coef), *grid)), H(y0).reshape(1, -1), tab,
                       [T1 / 3] * 3).reshape(2, 5, 7), torch.float64, "plain stencil y1")


def test_the_second_identical_solve_on_an_affine_operator_is_replayed_with_equal_bits():
    grid = (5, 7)
    op = AffineOp(StencilOp(grid, _stencil(), form="heat", boundary="neumann"))
    rng = np.random.default_rng(17)
    cparams = op.constrain(T(rng.uniform(0.3, 0.8, grid)), T(rng.standard_normal(35)))
    z0 = AffineOp.lift(T(rng.standard_normal((1, 35))))
    tab, dts = rk_tableaux.get("heun"), (T1 / 4,) * 4

    def run():
        y1, _ = pde_util._rk_forward(op, cparams, tab, dts, z0, False)
        torch.cuda.synchronize()
        return y1

    cap0, rep0 = _lib.graph_stats()
    first = run()
    ref = first.clone()
    del first  # the output goes back to the allocator: the next call gets the same address
    for _ in range(3):
        again = run()
        assert torch.equal(again, ref)
        del again
    cap1, rep1 = _lib.graph_stats()
    assert cap1 - cap0 >= 1 and rep1 - rep0 >= 2, "the second call is captured, the later ones replay"
