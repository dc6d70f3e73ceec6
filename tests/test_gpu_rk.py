"""The fixed-step Runge-Kutta drivers on the GPU (csrc/mfx_rk.hip through util/pde_util.solver_rk) against the fp64 restatement
(tests/_rk_restatement.py): forward, the discrete adjoint (autograd of the restatement) and the backsolve adjoint (the restated
backsolve recursion -- not the discrete gradient, from which it legitimately differs).

Tolerances: the project's parity tolerances, 1e-10 in fp64 and 1e-4 in fp32 of the largest entry of the
restated quantity.  Step sizes are stable: weights of O(1) (dx = 1), t1 - t0 = 1, 8 steps, so dt |A| <= 1.  Stencil grids: 1 x 1,
1 x 70, 17 x 65 and 33 x 130 around the 16-row x 64-column tile of the stencil kernels; at 33 x 130 the dense matrix (8580^2) is
not assembled and the restatement runs matrix-free (held against the dense one in tests/test_rk_host.py)."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _guarded_ws
import _rk_restatement as rr
import _stencil_restatement as sr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib
    from matfree_extensions.operators import CallbackOp, CsrOp, DenseOp, StencilOp
    from matfree_extensions.util import pde_util, rk_tableaux

DEV = torch.device("cuda:0")
METHODS = ("euler", "heun", "midpoint", "rk4", "dopri5", "dopri8")
GRIDS = [(1, 1), (1, 70), (17, 65), (33, 130)]
DTYPES = [torch.float64, torch.float32]
TOL = {torch.float64: 1e-10, torch.float32: 1e-4}
STEPS = 8
P = 3


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def H(t):
    return t.detach().cpu().to(torch.float64)


def rounded(x, dtype):
    """the fp64 value of x after rounding to dtype: what the device really sees"""
    return torch.tensor(np.asarray(x)).to(dtype).to(torch.float64)


def close(got, want, dtype, what):
    want = want if torch.is_tensor(want) else torch.tensor(np.asarray(want))
    err, scale = float((H(got).reshape(want.shape) - want).abs().max()), float(want.abs().max())
    print(f"{what}: max error {err:.3e}, largest entry {scale:.3e}, ratio {err / max(scale, 1e-300):.3e}")
    assert err <= TOL[dtype] * scale, (what, dtype, err, scale)


@functools.lru_cache(maxsize=None)
def _stencil():
    return pde_util.stencil_advection_diffusion(1.0).numpy()


def _field(ny, nx):
    return np.random.default_rng(100 * ny + nx).uniform(0.3, 0.8, (ny, nx))


def _states(n, seed, count=P):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((count, n)), rng.standard_normal((count, n))


def _run(solver, y0, params, w):
    """(y1, dy0, parameter gradients) of one solve and its backward with cotangent w"""
    y1, info = solver(y0, *params)
    grads = torch.autograd.grad(y1, [y0, *params], w)
    return y1.detach(), grads[0], grads[1:], info


# ---- forward and both adjoints, every method ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_dense_and_ragged_csr_against_the_restatement(kind, dtype):
    n = 37 if kind == "dense" else 150
    if kind == "dense":
        A64 = rounded(0.8 * np.random.default_rng(1).standard_normal((n, n)) / np.sqrt(n), dtype)
        op, theta = DenseOp(), T(A64, dtype, grad=True)
        grad_of = lambda dA: dA  # noqa: E731
    else:
        row, col, vals, _ = rr.csr_case(n, 2)
        op, vt, order = CsrOp.from_coo(row, col, vals, n, DEV)
        order = order.numpy()
        vals64 = rounded(vals[order], dtype)
        A64 = torch.tensor(rr.rc.dense_of(row[order], col[order], vals64.numpy(), n))
        theta = T(vals64, dtype, grad=True)
        grad_of = lambda dA: dA[row[order], col[order]]  # noqa: E731
    y0n, wn = _states(n, 3)
    y064, w64 = rounded(y0n, dtype), rounded(wn, dtype)
    dts = [1.0 / STEPS] * STEPS
    for method in METHODS:
        tab = rk_tableaux.get(method)
        ref_y1, ref_dy0, ref_dA = rr.discrete_gradients(A64, y064, tab, dts, w64)
        bs_dy0, bs_dA = rr.backsolve(A64, ref_y1, w64, tab, dts)
        for adjoint, (want0, wantA) in (("discrete", (ref_dy0, ref_dA)), ("backsolve", (bs_dy0, bs_dA))):
            solver = pde_util.solver_rk(0.0, 1.0, op, num_steps=STEPS, method=method, adjoint=adjoint)
            y1, dy0, (dth,), info = _run(solver, T(y064, dtype, grad=True), (theta,), T(w64, dtype))
            assert info == {"num_matvecs": STEPS * tab.order, "num_applies": STEPS * len(tab.b)}
            close(y1, ref_y1, dtype, f"{kind} {method} y1")
            close(dy0, want0, dtype, f"{kind} {method} {adjoint} dy0")
            close(dth, grad_of(wantA), dtype, f"{kind} {method} {adjoint} dtheta")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("boundary", sr.BOUNDARIES)
@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_stencil_against_the_restatement(grid, form, boundary, dtype):
    ny, nx = grid
    st = _stencil()
    coef64 = rounded(_field(ny, nx), dtype)
    st_dev = rounded(st, dtype).numpy()  # the weights are rounded to the dtype on their way into the kernel arguments
    op = StencilOp(grid, st, form=form, boundary=boundary)
    n = op.n
    y0n, wn = _states(n, 5)
    y064, w64 = rounded(y0n, dtype), rounded(wn, dtype)
    dts = [1.0 / STEPS] * STEPS
    dense = ny * nx <= 2000
    if dense:
        A64 = torch.tensor(rr.stencil_case(form, st_dev, boundary, coef64.numpy(), ny, nx))
    else:
        apply = rr.torch_stencil_apply(form, st_dev, boundary, ny, nx)
    for method in METHODS:
        tab = rk_tableaux.get(method)
        if dense:
            ref_y1, ref_dy0, dA = rr.discrete_gradients(A64, y064, tab, dts, w64)
            ref_dc = rr.stencil_gradient(form, st_dev, boundary, dA.numpy(), ny, nx)
            bs_dy0, bA = rr.backsolve(A64, ref_y1, w64, tab, dts)
            bs_dc = rr.stencil_gradient(form, st_dev, boundary, bA.numpy(), ny, nx)
        else:
            ref_y1, ref_dy0, ref_dc = rr.discrete_gradients_fn(apply, coef64, y064, tab, dts, w64)
            bs_dy0, bs_dc = rr.backsolve_fn(apply, coef64, ref_y1, w64, tab, dts)
        for adjoint, (want0, wantc) in (("discrete", (ref_dy0, ref_dc)), ("backsolve", (bs_dy0, bs_dc))):
            solver = pde_util.solver_rk(0.0, 1.0, op, num_steps=STEPS, method=method, adjoint=adjoint)
            y1, dy0, (dc,), _ = _run(solver, T(y064, dtype, grad=True), (T(coef64, dtype, grad=True),), T(w64, dtype))
            close(y1, ref_y1, dtype, f"{form} {boundary} {method} y1")
            close(dy0, want0, dtype, f"{form} {boundary} {method} {adjoint} dy0")
            close(dc, wantc, dtype, f"{form} {boundary} {method} {adjoint} dcoef")


# ---- batch, padding, ys, non-uniform steps, dy0 = NULL -------------------------------------------------------------------------
def _raw_solve(op, cparams, tab, dts, Y0pad, n, ldy1, keep_ys, sentinel=7.5, ws=None):
    lib = _lib.get()
    p, dt = Y0pad.shape[0], Y0pad.dtype
    desc = op.descriptor(cparams, dt, n)
    ts = rk_tableaux.struct(tab)
    y1 = torch.full((p, ldy1), sentinel, dtype=dt, device=DEV)
    ys = torch.empty((p, len(dts) + 1, n), dtype=dt, device=DEV) if keep_ys else None
    if ws is None:
        ws = _lib.scratch(int(lib.mfx_rk_workspace_bytes(C.byref(desc), C.byref(ts), n, p, 0)), DEV)
    rc = lib.mfx_rk_solve(C.byref(desc), C.byref(ts), (C.c_double * len(dts))(*dts), len(dts), _lib.ptr(Y0pad), Y0pad.stride(0), n, p,
                          _lib.ptr(y1), ldy1, _lib.ptr(ys), 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    return rc, y1, ys


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_batch_with_padded_leading_dimensions_and_the_iterates(dtype):
    grid = (17, 65)
    op = StencilOp(grid, _stencil(), form="wave", boundary="neumann")
    n = op.n
    coef = T(_field(*grid), dtype)
    y0n, _ = _states(n, 8)
    tab, dts = rk_tableaux.get("rk4"), [1.0 / STEPS] * STEPS
    for pad0, pad1 in ((5, 3), (2, 6)):  # odd paddings: the 16-byte loads must fall back where a row is not aligned
        Y0 = torch.full((P, n + pad0), -3.25, dtype=dtype, device=DEV)
        Y0[:, :n] = T(y0n, dtype)
        rc, y1, ys = _raw_solve(op, op.constrain(coef), tab, dts, Y0, n, n + pad1, True)
        assert rc == 0
        assert torch.all(y1[:, n:] == 7.5) and torch.all(Y0[:, n:] == -3.25)  # the sentinels survive
        assert torch.equal(ys[:, 0], Y0[:, :n]) and torch.equal(ys[:, -1], y1[:, :n])
        want, want_ys = rr.solve(torch.tensor(rr.stencil_case("wave", rounded(_stencil(), dtype).numpy(), "neumann", H(coef).numpy(),
                                                              *grid)), H(Y0[:, :n]), tab, dts, return_ys=True)
        close(y1[:, :n], want, dtype, "padded y1")
        close(ys, want_ys, dtype, "ys")
        # without ys the result is the same bits
        rc, y1b, _ = _raw_solve(op, op.constrain(coef), tab, dts, Y0, n, n + pad1, False)
        assert rc == 0 and torch.equal(y1b, y1)


def test_solver_euler_takes_a_non_uniform_grid_and_a_state_of_any_shape():
    ny, nx = 17, 65
    st = _stencil()
    coef = T(_field(ny, nx), grad=True)
    par, _ = pde_util.pde_wave_anisotropic(coef.detach(), st, constrain=lambda s: s, boundary=pde_util.boundary_neumann())
    ts = np.cumsum([0.0, 0.05, 0.2, 0.1, 0.15, 0.12, 0.08, 0.18, 0.12])
    rng = np.random.default_rng(9)
    y0n, wn = rng.standard_normal((2, ny, nx)), rng.standard_normal((2, ny, nx))
    A = torch.tensor(rr.stencil_case("wave", st, "neumann", H(coef).numpy(), ny, nx))
    tab = rk_tableaux.get("euler")
    ref_y1, ref_dy0, dA = rr.discrete_gradients(A, torch.tensor(y0n).reshape(1, -1), tab, np.diff(ts), torch.tensor(wn).reshape(1, -1))
    solve = pde_util.solver_euler(ts, par(scale=coef).flat)
    y0 = T(y0n, grad=True)
    y1, info = solve(y0)
    assert y1.shape == (2, ny, nx) and info["num_applies"] == 8
    dy0, dc = torch.autograd.grad(y1, [y0, coef], T(wn))
    close(y1, ref_y1.reshape(2, ny, nx), torch.float64, "euler y1")
    close(dy0, ref_dy0.reshape(2, ny, nx), torch.float64, "euler dy0")
    close(dc, rr.stencil_gradient("wave", st, "neumann", dA.numpy(), ny, nx), torch.float64, "euler dcoef")
    # a batch: one more dimension than the operator's state
    yb = T(np.stack([y0n, 2 * y0n, -y0n]))
    assert torch.equal(solve(yb)[0][0], y1.detach())


@pytest.mark.parametrize("adjoint", ["discrete", "backsolve"])
def test_parameter_gradients_do_not_depend_on_dy0(adjoint):
    n = 37
    A = T(0.8 * np.random.default_rng(1).standard_normal((n, n)) / np.sqrt(n), grad=True)
    y0n, wn = _states(n, 3)
    solver = pde_util.solver_rk(0.0, 1.0, DenseOp(), num_steps=STEPS, method="dopri5", adjoint=adjoint)
    (with0,) = _run(solver, T(y0n, grad=True), (A,), T(wn))[2]
    y1, _ = solver(T(y0n), A)  # y0 needs no gradient: dy0 = NULL
    (without,) = torch.autograd.grad(y1, [A], T(wn))
    assert torch.equal(with0, without)


# ---- graph replay ----------------------------------------------------------------------------------------------------------------
def test_graph_replay_and_its_key():
    n = 37
    A64 = torch.tensor(0.8 * np.random.default_rng(1).standard_normal((n, n)) / np.sqrt(n))
    A = T(A64)
    y0n, _ = _states(n, 3)
    y0 = T(y0n)

    def run(tab, dts):
        y1, _ = pde_util._rk_forward(DenseOp(), (A,), tab, tuple(dts), y0, False)
        torch.cuda.synchronize()
        return y1

    heun, midpoint = rk_tableaux.get("heun"), rk_tableaux.get("midpoint")
    dts = [1.0 / STEPS] * STEPS
    cap0, rep0 = _lib.graph_stats()
    first = run(heun, dts)
    ref = first.clone()
    del first  # the output goes back to the allocator: the next call gets the same address
    for _ in range(3):
        again = run(heun, dts)
        assert torch.equal(again, ref)
        del again
    cap1, rep1 = _lib.graph_stats()
    assert cap1 - cap0 >= 1 and rep1 - rep0 >= 2, "the second call is captured, the later ones replay"
    close(ref, rr.solve(A64, torch.tensor(y0n), heun, dts), torch.float64, "replayed heun")
    # the same nsteps, ONE different step size: the key changes, the result is the restatement's new one
    dts2 = list(dts)
    dts2[3] = 0.5 / STEPS
    for _ in range(3):
        got = run(heun, dts2)
        close(got, rr.solve(A64, torch.tensor(y0n), heun, dts2), torch.float64, "one changed step")
        assert not torch.equal(got, ref)
        del got
    # another tableau with the same stage count
    for _ in range(3):
        got = run(midpoint, dts)
        close(got, rr.solve(A64, torch.tensor(y0n), midpoint, dts), torch.float64, "midpoint after heun")
        del got
    assert torch.equal(run(heun, dts), ref)


# ---- workspace contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["stencil", "dense"])
def test_exact_guarded_poisoned_workspace(kind, monkeypatch):
    if kind == "stencil":
        grid = (17, 65)
        op, params = StencilOp(grid, _stencil(), form="wave", boundary="neumann"), (T(_field(*grid), grad=True),)
        n = op.n
    else:
        n = 37
        op, params = DenseOp(), (T(0.8 * np.random.default_rng(1).standard_normal((n, n)) / np.sqrt(n), grad=True),)
    y0n, wn = _states(n, 3)
    results = []
    for poison in (0x00, 0xFF):
        guard = _guarded_ws.GuardedWs(poison, busy=_lib._ws_busy)
        monkeypatch.setattr(_lib, "_take", guard.take)
        out = []
        for adjoint in ("discrete", "backsolve"):  # mfx_rk_solve with and without ys, mfx_rk_adjoint, mfx_rk_backsolve
            solver = pde_util.solver_rk(0.0, 1.0, op, num_steps=STEPS, method="dopri5", adjoint=adjoint)
            y1, dy0, grads, _ = _run(solver, T(y0n, grad=True), params, T(wn))
            out += [y1, dy0, *grads]
        guard.verify()
        assert guard.handed_out >= 4 and all(bool(torch.isfinite(t).all()) for t in out)
        results.append(out)
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_short_workspace_is_refused_with_everything_untouched():
    lib = _lib.get()
    n = 37
    A = T(np.eye(n))
    desc = DenseOp().descriptor((A,), torch.float64, n)
    ts = rk_tableaux.struct(rk_tableaux.get("rk4"))
    dts = (C.c_double * 2)(0.5, 0.5)
    buf = torch.full((4096,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = buf[1024 : 1024 + 255]
    y0, dy1 = T(np.ones((1, n))), T(np.ones((1, n)))
    out = torch.full((1, n), 7.5, dtype=torch.float64, device=DEV)
    ys = torch.full((1, 3, n), 7.5, dtype=torch.float64, device=DEV)
    g = _lib.OpGrads()
    gA = torch.zeros_like(A)
    g.dense_a = gA.data_ptr()
    st = _lib.stream_ptr(DEV)
    assert lib.mfx_rk_solve(C.byref(desc), C.byref(ts), dts, 2, _lib.ptr(y0), n, n, 1, _lib.ptr(out), n, None, 0, _lib.ptr(ws), 255, st) == -4
    assert lib.mfx_rk_adjoint(C.byref(desc), C.byref(ts), dts, 2, _lib.ptr(ys), n, 1, _lib.ptr(dy1), n, _lib.ptr(out), n, C.byref(g), 0,
                              _lib.ptr(ws), 255, st) == -4
    assert lib.mfx_rk_backsolve(C.byref(desc), C.byref(ts), dts, 2, _lib.ptr(y0), n, n, 1, _lib.ptr(dy1), n, _lib.ptr(out), n, C.byref(g), 0,
                                _lib.ptr(ws), 255, st) == -4
    torch.cuda.synchronize()
    assert torch.all(buf == 0xAB) and torch.all(out == 7.5) and torch.all(gA == 0)


# ---- refusals and the callback contract ------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    lib = _lib.get()
    n = 37
    A = T(np.eye(n))
    y0 = T(np.ones(n))
    with pytest.raises(TypeError, match="linear operator"):
        pde_util.solver_rk(0.0, 1.0, lambda v: A @ v, num_steps=4, method="rk4")
    with pytest.raises(ValueError, match="does not match"):
        pde_util.solver_rk(0.0, 1.0, DenseOp(), num_steps=4, method="rk4")(T(np.ones(n + 1)), A)
    desc = DenseOp().descriptor((A,), torch.float64, n)
    ts = rk_tableaux.struct(rk_tableaux.get("rk4"))
    ws = _lib.scratch(int(lib.mfx_rk_workspace_bytes(C.byref(desc), C.byref(ts), n, 1, 2)), DEV)
    out = torch.full((1, n), 7.5, dtype=torch.float64, device=DEV)
    dts = (C.c_double * 1)(0.5)
    st = _lib.stream_ptr(DEV)
    assert lib.mfx_rk_solve(C.byref(desc), C.byref(ts), dts, 0, _lib.ptr(y0), n, n, 1, _lib.ptr(out), n, None, 0, _lib.ptr(ws), ws.numel(), st) == -1
    gx = _lib.OpGrads()
    gx.x = out.data_ptr()
    for entry, lead in ((lib.mfx_rk_adjoint, (_lib.ptr(y0), n, 1)), (lib.mfx_rk_backsolve, (_lib.ptr(y0), n, n, 1))):
        assert entry(C.byref(desc), C.byref(ts), dts, 1, *lead, _lib.ptr(y0), n, _lib.ptr(out), n, C.byref(gx), 0, _lib.ptr(ws), ws.numel(), st) == -2
    rows = DenseOp().descriptor((A,), torch.float64, n)
    rows.nrows = 8
    assert lib.mfx_rk_solve(C.byref(rows), C.byref(ts), dts, 1, _lib.ptr(y0), n, n, 1, _lib.ptr(out), n, None, 0, _lib.ptr(ws), ws.numel(), st) == -2
    torch.cuda.synchronize()
    assert torch.all(out == 7.5)


@pytest.mark.parametrize("adjoint", ["discrete", "backsolve"])
def test_callback_operator_matches_the_native_one_and_surfaces_its_exception(adjoint):
    n = 37
    A64 = torch.tensor(0.8 * np.random.default_rng(1).standard_normal((n, n)) / np.sqrt(n))
    y0n, wn = _states(n, 3, count=1)
    tab, dts = rk_tableaux.get("rk4"), [1.0 / STEPS] * STEPS
    ref_y1, ref_dy0, ref_dA = rr.discrete_gradients(A64, torch.tensor(y0n), tab, dts, torch.tensor(wn))
    if adjoint == "backsolve":
        ref_dy0, ref_dA = rr.backsolve(A64, ref_y1, torch.tensor(wn), tab, dts)
    solver = pde_util.solver_rk(0.0, 1.0, CallbackOp(lambda v, M: M @ v), num_steps=STEPS, method="rk4", adjoint=adjoint)
    y1, dy0, (dA,), _ = _run(solver, T(y0n[0], grad=True), (T(A64, grad=True),), T(wn[0]))
    close(y1, ref_y1[0], torch.float64, "callback y1")
    close(dy0, ref_dy0[0], torch.float64, f"callback {adjoint} dy0")
    close(dA, ref_dA, torch.float64, f"callback {adjoint} dA")

    class Boom(Exception):
        pass

    def broken(v, M):
        raise Boom("inside the matvec")

    with pytest.raises(Boom, match="inside the matvec"):
        pde_util.solver_rk(0.0, 1.0, CallbackOp(broken), num_steps=2, method="heun", adjoint=adjoint)(T(y0n[0]), T(A64))
