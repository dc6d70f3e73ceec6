"""The adaptive-step Runge-Kutta solve on the GPU (mfx_rk_solve_adaptive through util/pde_util.solver_rk_adaptive) against the NumPy
restatement of scheme and controller (tests/_rk_adaptive_restatement.py) and against the fixed-step driver on the accepted steps.

Cases: the heat operator c = 1, 5-point Laplacian / dx^2, Dirichlet boundary, t in [0, 0.1], dt0 = 0.1 / 9, atol = 1e-8,
y0 = default_rng(0).standard_normal(n); 8 x 8 (dx = 1/7) and 7 x 5 (dx = 1/6), rtol 1e-3 and 1e-6.  Every parity test first asserts
ON THE RESTATEMENT that no accept / reject decision lies within 1 % of a tie (a condition on the inputs, not a tolerance on the code).

Bounds on dts and y1 against the restatement: the counts are exact; the values differ because the device
fuses multiply-adds and its pow is not libm's, and a difference in one norm moves every later step (in fp32 at rtol = 1e-6 the
error estimate is itself only a few digits above the rounding of the stages).  Measured on the first run, largest over all cases,
relative to the largest entry: fp64 dts 7.3e-12, y1 1.1e-14; fp32 dts 1.2e-2, y1 1.1e-5.  The bounds are 10 x those figures per
dtype."""

import math

import numpy as np
import pytest
import torch

import _guarded_ws
import _rk_adaptive_restatement as ar

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib
    from matfree_extensions.operators import AffineOp, DenseOp, StencilOp
    from matfree_extensions.util import pde_util, rk_tableaux

DEV = torch.device("cuda:0")
T0, T1, DT0, ATOL = 0.0, 0.1, 0.1 / 9, 1e-8
GRIDS = {"8x8": ((8, 8), 1 / 7), "7x5": ((7, 5), 1 / 6)}
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
DTS_TOL = {torch.float64: 7.3e-11, torch.float32: 1.2e-1}
Y1_TOL = {torch.float64: 1.1e-13, torch.float32: 1.1e-4}
BACKSOLVE_TOL = 1e-10  # tests/test_gpu_rk.py: backsolve in fp64, relative to the largest entry
_MEASURED = {}


def T(x, dtype=torch.float64, grad=False):
    t = torch.tensor(np.asarray(x), dtype=dtype, device=DEV)
    return t.requires_grad_(True) if grad else t


def H(t):
    return t.detach().cpu().to(torch.float64).numpy()


def _pair():
    return rk_tableaux.get_pair("dopri5")


def _heat(grid_id):
    (ny, nx), dx = GRIDS[grid_id]
    return (ny, nx), dx, ar.heat_matrix(ny, nx, dx), np.random.default_rng(0).standard_normal(ny * nx)


def _stencil_op(grid, dx, form="heat", sign=1.0):
    """the 5-point Laplacian / dx^2 (centre -4: not pde_util.stencil_laplacian, whose centre is the reference's -2)"""
    lap = np.array([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]]) / dx**2
    return StencilOp(grid, sign * lap, form=form, boundary="dirichlet")


def _batch(y0, p):
    return np.stack([y0, 10.0 * y0, 0.1 * y0][:p])


def _solver(op, rtol, **kw):
    return pde_util.solver_rk_adaptive(T0, T1, op, method="dopri5", rtol=rtol, atol=ATOL, dt0=DT0, **kw)


def _check_parity(got_y1, info, ref, dtype, what):
    assert ref["status"] == ar.OK and ar.clear_of_ties(ref), "the case itself must stay 1 % clear of a tie"
    assert (info["num_steps"], info["num_rejected"]) == (ref["n_accepted"], ref["n_rejected"]), what
    assert info["status"] == "ok" and info["num_applies"] == 7 * (ref["n_accepted"] + ref["n_rejected"])
    assert info["num_matvecs"] == 5 * ref["n_accepted"]
    dts = np.array(info["dts"])
    assert math.fsum(dts) == T1 - T0, (what, math.fsum(dts))
    ddts = float(np.abs(dts - ref["dts"]).max() / ref["dts"].max())
    dy1 = float(np.abs(H(got_y1).reshape(ref["y1"].shape) - ref["y1"]).max() / np.abs(ref["y1"]).max())
    print(f"{what}: {info['num_steps']} + {info['num_rejected']} steps, dts off by {ddts:.3e}, y1 off by {dy1:.3e} (relative to the largest)")
    key = str(dtype)
    _MEASURED[key] = (max(_MEASURED.get(key, (0, 0))[0], ddts), max(_MEASURED.get(key, (0, 0))[1], dy1))
    print(f"   largest so far for {key}: dts {_MEASURED[key][0]:.3e}, y1 {_MEASURED[key][1]:.3e}")
    assert ddts <= DTS_TOL[dtype] and dy1 <= Y1_TOL[dtype], (what, ddts, dy1)


# ---- 1. parity with the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("rtol", [1e-3, 1e-6])
@pytest.mark.parametrize("grid_id", list(GRIDS))
def test_stencil_and_dense_take_the_restatements_steps(grid_id, rtol, p, dtype):
    grid, dx, A, y0 = _heat(grid_id)
    A_dev = T(A, dtype)  # the weights 1 / dx^2 are rounded to the dtype on their way in: the restatement gets the rounded matrix
    Y0 = T(_batch(y0, p), dtype)
    ref = ar.solve(H(A_dev), H(Y0), _pair(), T0, T1, DT0, rtol, ATOL, dtype=NP[dtype])
    if dtype == torch.float64 and p == 1:
        want = {("8x8", 1e-3): (17, 3), ("8x8", 1e-6): (46, 2), ("7x5", 1e-3): (13, 1), ("7x5", 1e-6): (40, 2)}[(grid_id, rtol)]
        assert (ref["n_accepted"], ref["n_rejected"]) == want
    y0_in = Y0[0] if p == 1 else Y0
    y1, info = _solver(_stencil_op(grid, dx), rtol)(y0_in)
    assert y1.shape == y0_in.shape
    _check_parity(y1, info, ref, dtype, f"stencil {grid_id} rtol {rtol} p {p} {dtype}")
    y1d, infod = _solver(DenseOp(), rtol)(y0_in, A_dev)
    _check_parity(y1d, infod, ref, dtype, f"dense {grid_id} rtol {rtol} p {p} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1027, 1028])
@pytest.mark.parametrize("p", [1, 3])
def test_zero_padded_state_over_several_blocks(p, n, dtype):
    """the 8 x 8 state inside n = 1027 (odd: scalar access, three blocks, a ragged last one) and 1028 (16-byte access, a ragged tail)"""
    _, _, A, y0 = _heat("8x8")
    Abig, ybig = np.zeros((n, n)), np.zeros(n)
    Abig[:64, :64], ybig[:64] = A, y0
    A_dev, Y0 = T(Abig, dtype), T(_batch(ybig, p), dtype)
    for rtol in (1e-3, 1e-6):
        ref = ar.solve(H(A_dev), H(Y0), _pair(), T0, T1, DT0, rtol, ATOL, dtype=NP[dtype])
        y1, info = _solver(DenseOp(), rtol)(Y0[0] if p == 1 else Y0, A_dev)
        _check_parity(y1, info, ref, dtype, f"padded n {n} rtol {rtol} p {p} {dtype}")
        assert torch.all(y1.reshape(p, n)[:, 64:] == 0)


# ---- 2. bit identity with the fixed-step driver on the accepted steps --------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["stencil", "dense"])
def test_accepted_iterates_are_the_fixed_step_drivers(kind, dtype):
    grid, dx, A, y0 = _heat("7x5")
    op, params = (_stencil_op(grid, dx), ()) if kind == "stencil" else (DenseOp(), (T(A, dtype),))
    Y0 = T(_batch(y0, 3), dtype)
    y1, info = _solver(op, 1e-6)(Y0, *params)
    fixed, _ = pde_util._rk_solver(info["dts"], op, "dopri5", "discrete")(Y0, *params)
    assert torch.equal(y1, fixed)
    cparams = op.constrain(*params)
    cfg = {"t0": T0, "t1": T1, "dt0": DT0, "rtol": 1e-6, "atol": ATOL, "max_steps": 100}
    y1k, ys, dts, st = pde_util._rk_adaptive_forward(op, cparams, _pair(), cfg, Y0, True)
    y1f, ysf = pde_util._rk_forward(op, cparams, rk_tableaux.get("dopri5"), dts, Y0, True)
    assert dts == info["dts"] and st.t_reached == T1 and st.n_attempts == info["num_steps"] + info["num_rejected"]
    assert ys.shape == ysf.shape == (3, len(dts) + 1, Y0.shape[1])
    assert torch.equal(ys, ysf) and torch.equal(y1k, y1f) and torch.equal(y1k, y1) and torch.equal(ys[:, 0], Y0)


# ---- 3. chunks, repeats, no stale graph -----------------------------------------------------------------------------------------------
def test_chunks_repeats_and_another_tolerance_on_the_same_buffers():
    grid, dx, A, y0 = _heat("8x8")
    op, Y0 = _stencil_op(grid, dx), T(_batch(y0, 3))
    counts = {}
    for rtol in (1e-3, 1e-6):
        ref = ar.solve(A, _batch(y0, 3), _pair(), T0, T1, DT0, rtol, ATOL)
        assert ar.clear_of_ties(ref)
        counts[rtol] = (ref["n_accepted"], ref["n_rejected"])
    assert counts[1e-3] != counts[1e-6]
    cap0, rep0 = _lib.graph_stats()
    solve = {rtol: _solver(op, rtol) for rtol in counts}
    first = {}
    for _ in range(3):  # the tolerances alternate on the same workspace and the same graph cache
        for rtol in counts:
            for chunk in (8, 1, 3):
                y1, info = solve[rtol](Y0, chunk=chunk)
                assert (info["num_steps"], info["num_rejected"]) == counts[rtol], (rtol, chunk)
                if rtol not in first:
                    first[rtol] = (y1.clone(), info["dts"])
                assert torch.equal(y1, first[rtol][0]) and info["dts"] == first[rtol][1], (rtol, chunk)
                del y1
    cap1, rep1 = _lib.graph_stats()
    assert cap1 - cap0 >= 1 and rep1 - rep0 >= 2, "a chunk is captured on its second sighting and replayed afterwards"
    assert not torch.equal(first[1e-3][0], first[1e-6][0])


# ---- 4. stability ---------------------------------------------------------------------------------------------------------------------
def test_fixed_steps_blow_up_where_the_controller_does_not():
    grid, dx, A, y0 = _heat("8x8")
    op, y0t = _stencil_op(grid, dx), T(y0)
    fixed, _ = pde_util.solver_rk(T0, T1, op, num_steps=9, method="dopri5")(y0t)
    assert float(fixed.abs().max()) > 1e3
    exact = H(torch.linalg.matrix_exp(T(T1 * A)) @ y0t)
    assert np.abs(exact).max() < 0.03
    for rtol in (1e-3, 1e-6):
        ref_err = np.abs(ar.solve(A, y0, _pair(), T0, T1, DT0, rtol, ATOL)["y1"][0] - exact).max()
        y1, _ = _solver(op, rtol)(y0t)
        err = np.abs(H(y1) - exact).max()
        print(f"rtol {rtol}: error against matrix_exp {err:.3e}, the restatement's {ref_err:.3e}")
        assert err <= 10 * ref_err


def test_initial_step_rule_and_the_other_pairs():
    from scipy.integrate import solve_ivp

    grid, dx, A, y0 = _heat("7x5")
    op, y0t = _stencil_op(grid, dx), T(y0)
    for method, name, stages in (("RK45", "dopri5", 7), ("RK23", "bosh3", 4)):
        sol = solve_ivp(lambda t, y: A @ y, (T0, T1), y0, method=method, rtol=1e-4, atol=ATOL)
        y1, info = pde_util.solver_rk_adaptive(T0, T1, op, method=name, rtol=1e-4, atol=ATOL)(y0t)
        print(f"{name}: scipy {len(sol.t) - 1} steps, first {sol.t[1]:.6e}; device {info['num_steps']} steps, first {info['dts'][0]:.6e}")
        assert abs(info["dts"][0] - sol.t[1]) <= 1e-9 * sol.t[1] and abs(info["num_steps"] - (len(sol.t) - 1)) <= 1
        assert info["num_applies"] == stages * (info["num_steps"] + info["num_rejected"])
        assert np.abs(H(y1) - sol.y[:, -1]).max() <= 1e-3 * np.abs(y0).max()
    y1, info = pde_util.solver_rk_adaptive(T0, T1, op, method="heun", rtol=1e-2, atol=1e-4, dt0=DT0)(y0t)
    ref = ar.solve(A, y0, rk_tableaux.get_pair("heun"), T0, T1, DT0, 1e-2, 1e-4)
    assert ar.clear_of_ties(ref, 1e-3)
    assert (info["num_steps"], info["num_rejected"]) == (ref["n_accepted"], ref["n_rejected"])
    assert np.abs(H(y1) - ref["y1"][0]).max() <= 1e-9 * np.abs(ref["y1"]).max()


# ---- 5. gradients: those of the fixed-step solve with the same dts ---------------------------------------------------------------------
def _grads(solver, y0, params, w):
    y1, info = solver(y0, *params)
    return (y1.detach(), info, *torch.autograd.grad(y1, [y0, *params], w))


@pytest.mark.parametrize("adjoint", ["discrete", "backsolve"])
@pytest.mark.parametrize("case", ["heat2", "affine"])
def test_gradients_are_the_fixed_step_ones_on_the_accepted_steps(case, adjoint):
    grid, dx, _, _ = _heat("7x5")
    ny, nx = grid
    rng = np.random.default_rng(4)
    if case == "heat2":  # (u, du)' = (-coef o S u, du) with S = -Laplacian: the heat equation with a coefficient field, and du' = du
        op = _stencil_op(grid, dx, form="heat2", sign=-1.0)
        params = [T(rng.uniform(0.5, 1.0, (ny, nx)), grad=True)]
        n = 2 * ny * nx
    else:
        op = AffineOp(_stencil_op(grid, dx))
        params = [T(rng.standard_normal(ny * nx), grad=True)]
        n = ny * nx
    y0n, wn = rng.standard_normal((3, n)), rng.standard_normal((3, n))
    y1, info, dy0, dth = _grads(_solver(op, 1e-4, adjoint=adjoint), T(y0n, grad=True), params, T(wn))
    assert info["num_steps"] >= 5
    y1f, _, dy0f, dthf = _grads(pde_util._rk_solver(info["dts"], op, "dopri5", adjoint), T(y0n, grad=True), params, T(wn))
    assert torch.equal(y1, y1f)
    for got, want, what in ((dy0, dy0f, "dy0"), (dth, dthf, "dtheta")):
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"{case} {adjoint} {what}: differs by {err:.3e} of {scale:.3e}")
        assert scale > 0 and bool(torch.isfinite(got).all())
        if adjoint == "discrete":
            assert torch.equal(got, want), what
        else:
            assert err <= BACKSOLVE_TOL * scale, what


# ---- 6. status paths and the workspace contract -------------------------------------------------------------------------------------------
def test_max_attempts_raises_and_the_guards_stay_intact(monkeypatch):
    grid, dx, A, y0 = _heat("8x8")
    op, Y0 = _stencil_op(grid, dx), T(_batch(y0, 3))
    ref = ar.solve(A, _batch(y0, 3), _pair(), T0, T1, DT0, 1e-3, ATOL, max_attempts=5)
    assert ref["status"] == ar.MAX_ATTEMPTS
    results = []
    for poison in (0x00, 0xFF):
        guard = _guarded_ws.GuardedWs(poison, busy=_lib._ws_busy)
        monkeypatch.setattr(_lib, "_take", guard.take)
        with pytest.raises(RuntimeError, match=r"^max_attempts"):
            _solver(op, 1e-3, max_steps=5)(Y0)
        guard.verify()
        out = []
        for adjoint in ("discrete", "backsolve"):  # the whole solve and both backwards over exact-size poisoned scratch
            y0g = Y0.clone().requires_grad_(True)
            y1, info = _solver(op, 1e-3, adjoint=adjoint, max_steps=40)(y0g)
            out += [y1.detach(), torch.autograd.grad(y1, y0g, torch.ones_like(y1))[0], torch.tensor(info["dts"])]
        guard.verify()
        assert guard.handed_out >= 5 and all(bool(torch.isfinite(t).all()) for t in out)
        results.append(out)
    for a, b in zip(*results):
        assert torch.equal(a, b)
    # the raw entry: the state at t_reached, the counters, sentinels beyond n and beyond the accepted rows
    lib, n, p = _lib.get(), 64, 3
    import ctypes as C

    desc = op.descriptor(op.constrain(), torch.float64, n)
    ps = rk_tableaux.pair_struct(_pair())
    ws = _lib.scratch(int(lib.mfx_rk_adaptive_workspace_bytes(C.byref(desc), C.byref(ps), n, p, 8)), DEV)
    y1 = torch.full((p, n + 3), 7.5, dtype=torch.float64, device=DEV)
    ys = torch.full((p, 9, n), 7.5, dtype=torch.float64, device=DEV)
    dts, st = (C.c_double * 8)(), _lib.RkAdaptiveInfo()
    rc = lib.mfx_rk_solve_adaptive(C.byref(desc), C.byref(ps), T0, T1, DT0, 1e-3, ATOL, 8, 5, 8, _lib.ptr(Y0), n, n, p, _lib.ptr(y1), n + 3,
                                   _lib.ptr(ys), dts, C.byref(st), 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    assert rc == 0 and st.status == _lib.RK_MAX_ATTEMPTS and "max_attempts" in lib.mfx_last_error().decode()
    assert (st.n_accepted, st.n_rejected, st.n_attempts) == (ref["n_accepted"], ref["n_rejected"], 5) and st.t_reached < T1
    assert abs(st.t_reached - ref["ts"][-1]) <= DTS_TOL[torch.float64] * T1
    assert torch.all(y1[:, n:] == 7.5) and torch.equal(y1[:, :n], ys[:, st.n_accepted]) and torch.all(ys[:, st.n_accepted + 1 :] == 7.5)
    assert np.abs(H(y1[:, :n]) - ref["y1"]).max() <= Y1_TOL[torch.float64] * np.abs(ref["y1"]).max()
