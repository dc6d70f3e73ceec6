"""CPU-side checks of the fixed-step Runge-Kutta drivers (no GPU): the C-ABI surface, the named tableaux (consistency and observed
order), the restatement the GPU tests measure against, and the refusals that come before any launch."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _rk_restatement as rr
from matfree_extensions import _lib
from matfree_extensions.operators import DenseOp, RowShardedOp
from matfree_extensions.util import pde_util, rk_tableaux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mfx_rk_workspace_bytes", "mfx_rk_solve", "mfx_rk_adjoint", "mfx_rk_backsolve"]
FAKE = ctypes.c_void_p(64)  # never dereferenced
BIG = 1 << 40


def test_symbols_are_declared_mirrored_and_exported():
    lib = _lib.get()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, f"{name} is not in _lib.SYMBOLS"
        decl = re.search(rf"\b{name}\s*\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name
    assert lib.mfx_version() == 201 and re.search(r"#define MFX_VERSION 201\b", header)
    assert re.search(r"#define MFX_RK_MAX_STAGES 16\b", header) and _lib.RK_MAX_STAGES == 16
    # struct mfx_rk_tableau: int32 stages, double a[16][16], double b[16]
    T = _lib.RkTableau
    assert [f[0] for f in T._fields_] == ["stages", "a", "b"]
    assert (T.a.offset, T.b.offset, ctypes.sizeof(T)) == (8, 8 + 16 * 16 * 8, 8 + 16 * 16 * 8 + 16 * 8)
    src = open(os.path.join(ROOT, "experiments-lanczos-adjoints_amd", "csrc", "Makefile")).read()
    assert "mfx_rk.hip" in src


@pytest.mark.parametrize("name", rk_tableaux.NAMES)
def test_tableau_is_consistent_and_strictly_lower(name):
    tab = rk_tableaux.get(name)
    s = len(tab.b)
    assert 1 <= s <= 16 and len(tab.a) == s
    # s <= 16 terms of magnitude <= 45 (dopri8): |fl(sum) - sum| <= 16 * 2^-53 * sum |b_i| < 2e-14
    assert abs(sum(tab.b) - 1.0) <= 16 * 2.0**-53 * sum(abs(v) for v in tab.b)
    for i, row in enumerate(tab.a):
        assert len(row) == i, (name, i)  # only the entries left of the diagonal exist
    st = rk_tableaux.struct(tab)
    assert st.stages == s
    for i in range(16):
        for j in range(16):
            want = tab.a[i][j] if (i < s and j < i) else 0.0
            assert st.a[i][j] == want
        assert st.b[i] == (tab.b[i] if i < s else 0.0)


def test_tableau_names():
    assert set(rk_tableaux.NAMES) == {"euler", "heun", "midpoint", "rk4", "dopri5", "dopri8"}
    assert [rk_tableaux.get(n).order for n in ("euler", "heun", "midpoint", "rk4", "dopri5", "dopri8")] == [1, 2, 2, 4, 5, 8]
    with pytest.raises(NotImplementedError, match="tsit5"):
        rk_tableaux.get("tsit5")
    with pytest.raises(ValueError, match="unknown"):
        rk_tableaux.get("rk5")


def _scalar_error(tab, lam, nsteps):
    """|y_N - exp(lam)| for y' = lam y, y(0) = 1 over [0, 1] in NumPy (longdouble accumulates nothing here: plain fp64)"""
    h = 1.0 / nsteps
    y = 1.0
    for _ in range(nsteps):
        ks = []
        for i in range(len(tab.b)):
            Y = y + h * sum(tab.a[i][j] * ks[j] for j in range(i))
            ks.append(lam * Y)
        y = y + h * sum(b * k for b, k in zip(tab.b, ks))
    return abs(y - np.exp(lam))


@pytest.mark.parametrize("name", rk_tableaux.NAMES)
def test_observed_order_under_step_halving(name):
    """Every pair (n, 2 n) of step counts from n = 4 on (h |lam| <= 1 for both solves: the leading error term dominates) whose finer
    error is still above 1e-12 (round-off does not).  lam = -1; for the 8th-order method, whose error at n = 4 is already below
    that floor, lam = -4, which moves the same regime to larger errors."""
    tab = rk_tableaux.get(name)
    q = tab.order
    lam = -4.0 if q >= 8 else -1.0
    pairs = []
    n = 4
    while n <= 1024:
        e1, e2 = _scalar_error(tab, lam, n), _scalar_error(tab, lam, 2 * n)
        if e2 < 1e-12:
            break
        pairs.append((n, e1 / e2))
        n *= 2
    assert pairs, name
    for n, r in pairs:
        assert 2.0 ** (q - 0.5) <= r <= 2.0 ** (q + 0.5), (name, n, r, q)


@pytest.mark.parametrize("name", ["heun", "rk4", "dopri5"])
def test_restated_discrete_gradient_is_the_finite_difference_of_its_own_value(name):
    tab = rk_tableaux.get(name)
    rng = np.random.default_rng(3)
    n, p = 6, 2
    A = torch.tensor(0.5 * rng.standard_normal((n, n)))
    y0 = torch.tensor(rng.standard_normal((p, n)))
    w = torch.tensor(rng.standard_normal((p, n)))
    dts = [0.1, 0.15, 0.05, 0.2]
    _, dy0, dA = rr.discrete_gradients(A, y0, tab, dts, w)

    def value(A_, y_):
        return float((rr.solve(A_, y_, tab, dts) * w).sum())

    eps = 1e-6
    for _ in range(6):
        dirA, diry = torch.tensor(rng.standard_normal((n, n))), torch.tensor(rng.standard_normal((p, n)))
        fd = (value(A + eps * dirA, y0 + eps * diry) - value(A - eps * dirA, y0 - eps * diry)) / (2 * eps)
        an = float((dA * dirA).sum() + (dy0 * diry).sum())
        assert abs(fd - an) <= 1e-8 * max(1.0, abs(an)), (name, fd, an)


def test_restated_backsolve_converges_to_the_discrete_gradient():
    """the continuous adjoint differs from the discrete one by the discretisation error only: it shrinks at the method's order"""
    tab = rk_tableaux.get("heun")
    rng = np.random.default_rng(4)
    n = 6
    A = torch.tensor(0.5 * rng.standard_normal((n, n)))
    y0, w = torch.tensor(rng.standard_normal((1, n))), torch.tensor(rng.standard_normal((1, n)))
    gaps = []
    for steps in (8, 16, 32):
        dts = [1.0 / steps] * steps
        y1, dy0, dA = rr.discrete_gradients(A, y0, tab, dts, w)
        b0, bA = rr.backsolve(A, y1, w, tab, dts)
        gaps.append(float((bA - dA).abs().max() + (b0 - dy0).abs().max()))
    assert gaps[0] > gaps[1] > gaps[2] > 0.0 and gaps[0] / gaps[2] > 8.0


@pytest.mark.parametrize("boundary", ["dirichlet", "neumann"])
@pytest.mark.parametrize("form", ["heat", "heat2", "wave"])
def test_matrix_free_restatement_is_the_dense_one(form, boundary):
    """the torch stencil (used where the dense matrix is too large) against the dense matrix of tests/_stencil_restatement.py"""
    ny, nx = 5, 7
    rng = np.random.default_rng(8)
    st = pde_util.stencil_advection_diffusion(1.0).numpy()
    coef = rng.uniform(0.5, 1.5, (ny, nx))
    A = torch.tensor(rr.stencil_case(form, st, boundary, coef, ny, nx))
    n = A.shape[0]
    y0, w = torch.tensor(rng.standard_normal((2, n))), torch.tensor(rng.standard_normal((2, n)))
    tab, dts = rk_tableaux.get("rk4"), [0.125] * 8
    apply = rr.torch_stencil_apply(form, st, boundary, ny, nx)
    y1, dy0, dA = rr.discrete_gradients(A, y0, tab, dts, w)
    y1f, dy0f, dcf = rr.discrete_gradients_fn(apply, torch.tensor(coef), y0, tab, dts, w)
    scale = float(y1.abs().max())
    assert float((y1 - y1f).abs().max()) <= 1e-13 * scale and float((dy0 - dy0f).abs().max()) <= 1e-13 * float(dy0.abs().max())
    dc = rr.stencil_gradient(form, st, boundary, dA.numpy(), ny, nx)
    assert np.abs(dc - dcf.numpy()).max() <= 1e-13 * np.abs(dc).max()
    b0, bA = rr.backsolve(A, y1, w, tab, dts)
    b0f, bcf = rr.backsolve_fn(apply, torch.tensor(coef), y1, w, tab, dts)
    bc = rr.stencil_gradient(form, st, boundary, bA.numpy(), ny, nx)
    assert float((b0 - b0f).abs().max()) <= 1e-13 * float(b0.abs().max()) and np.abs(bc - bcf.numpy()).max() <= 1e-13 * np.abs(bc).max()


def _dense_desc(n=8):
    d = _lib.Operator()
    d.kind, d.dtype, d.n = _lib.OP_DENSE, _lib.MFX_F64, n
    d.dense_a, d.lda = 64, n
    return d


def _solve(lib, desc, tab, dts, n=8, p=1, ld=None, ws_bytes=BIG, flags=0):
    arr = (ctypes.c_double * max(len(dts), 1))(*dts)
    ld = n if ld is None else ld
    return lib.mfx_rk_solve(ctypes.byref(desc), ctypes.byref(tab), arr, len(dts), FAKE, ld, n, p, FAKE, ld, None, flags, FAKE, ws_bytes, None)


def test_refusals_come_before_any_launch():
    lib = _lib.get()
    good = rk_tableaux.struct(rk_tableaux.get("rk4"))
    desc = _dense_desc()

    def tab(**edit):
        t = rk_tableaux.struct(rk_tableaux.get("rk4"))
        for key, v in edit.items():
            if key == "stages":
                t.stages = v
            elif key == "a":
                t.a[v[0]][v[1]] = v[2]
            else:
                t.b[v[0]] = v[1]
        return t

    bad = [tab(stages=0), tab(stages=17), tab(stages=-1), tab(a=(1, 1, 0.5)), tab(a=(0, 2, 1e-300)), tab(a=(2, 2, 1.0)),
           tab(a=(2, 1, float("nan"))), tab(a=(3, 0, float("inf"))), tab(b=(1, float("nan")))]
    for t in bad:
        assert _solve(lib, desc, t, [0.1]) == -1, lib.mfx_last_error().decode()
        assert "tableau" in lib.mfx_last_error().decode()
        assert lib.mfx_rk_workspace_bytes(ctypes.byref(desc), ctypes.byref(t), 8, 1, 0) == -1 or 1 <= t.stages <= 16
    # the operator's own faults come first
    broken = _dense_desc()
    broken.dense_a = None
    assert _solve(lib, broken, tab(stages=0), [0.1]) == -1 and "dense operator without matrix" in lib.mfx_last_error().decode()
    # a row block
    rows = _dense_desc()
    rows.nrows = 4
    assert _solve(lib, rows, good, [0.1]) == -2 and "row-sharded" in lib.mfx_last_error().decode()
    assert _solve(lib, desc, good, []) == -1 and "nsteps" in lib.mfx_last_error().decode()
    assert _solve(lib, desc, good, [0.1], p=0) == -1
    assert _solve(lib, desc, good, [0.1], ld=7) == -1 and "leading" in lib.mfx_last_error().decode()
    assert _solve(lib, desc, good, [0.1], n=9) == -1
    assert _solve(lib, desc, good, [float("nan")]) == -1 and "dts" in lib.mfx_last_error().decode()
    assert _solve(lib, desc, good, [0.1], flags=6) == -1
    need = lib.mfx_rk_workspace_bytes(ctypes.byref(desc), ctypes.byref(good), 8, 1, 0)
    assert need > 0 and _solve(lib, desc, good, [0.1], ws_bytes=need - 1) == -4
    assert _solve(lib, desc, good, [0.1], ws_bytes=255) == -4
    sizes = [lib.mfx_rk_workspace_bytes(ctypes.byref(desc), ctypes.byref(good), 8, 1, m) for m in (0, 1, 2)]
    assert 0 < sizes[0] < sizes[1] <= sizes[2] and lib.mfx_rk_workspace_bytes(ctypes.byref(desc), ctypes.byref(good), 8, 1, 3) == -1
    # the adjoints: grads->x is refused, and so is a short workspace
    arr = (ctypes.c_double * 1)(0.1)
    gx = _lib.OpGrads()
    gx.dense_a = gx.x = 64
    g = _lib.OpGrads()
    g.dense_a = 64
    adj = lambda gr, wsb: lib.mfx_rk_adjoint(ctypes.byref(desc), ctypes.byref(good), arr, 1, FAKE, 8, 1, FAKE, 8, FAKE, 8,  # noqa: E731
                                             ctypes.byref(gr), 0, FAKE, wsb, None)
    back = lambda gr, wsb: lib.mfx_rk_backsolve(ctypes.byref(desc), ctypes.byref(good), arr, 1, FAKE, 8, 8, 1, FAKE, 8, FAKE, 8,  # noqa: E731
                                                ctypes.byref(gr), 0, FAKE, wsb, None)
    for call in (adj, back):
        assert call(gx, BIG) == -2 and "grads->x" in lib.mfx_last_error().decode()
        assert call(g, 255) == -4


def test_python_layer_refusals():
    with pytest.raises(TypeError, match="linear operator"):
        pde_util.solver_rk(0.0, 1.0, lambda v: v, num_steps=4, method="rk4")
    with pytest.raises(NotImplementedError, match="tsit5"):
        pde_util.solver_rk(0.0, 1.0, DenseOp(), num_steps=4, method="tsit5")
    with pytest.raises(ValueError, match="adjoint"):
        pde_util.solver_rk(0.0, 1.0, DenseOp(), num_steps=4, method="rk4", adjoint="forward")
    with pytest.raises(ValueError, match="num_steps"):
        pde_util.solver_rk(0.0, 1.0, DenseOp(), num_steps=0, method="rk4")
    sharded = RowShardedOp.__new__(RowShardedOp)  # refused by its type, before any collective could run
    sharded.op, sharded.comm, sharded.plans = DenseOp(), None, None
    with pytest.raises(NotImplementedError, match="row-sharded"):
        pde_util.solver_rk(0.0, 1.0, sharded, num_steps=4, method="rk4")
    assert pde_util.solver_diffrax is pde_util.solver_rk
    for name in ("recursive_checkpoint", "direct", "backsolve", "discrete"):
        pde_util.solver_rk(0.0, 1.0, DenseOp(), num_steps=4, method="heun", adjoint=name)
    # no tensor on a device: the solve itself refuses, there is no CPU path
    solve = pde_util.solver_euler([0.0, 0.5, 1.0], DenseOp())
    with pytest.raises(_lib.MfxError, match="ROCm device"):
        solve(torch.ones(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64))
