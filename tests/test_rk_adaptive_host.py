"""The adaptive-step Runge-Kutta solve without a GPU: the NumPy restatement of scheme and controller (tests/_rk_adaptive_restatement.py)
against scipy's solve_ivp, the literal pair coefficients against scipy's, and what mfx_rk_solve_adaptive refuses before any launch."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _rk_adaptive_restatement as ar
from matfree_extensions import _lib
from matfree_extensions.operators import DenseOp, RowShardedOp
from matfree_extensions.util import pde_util, rk_tableaux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(64)  # never dereferenced
BIG = 1 << 40
T0, T1, DT0, ATOL = 0.0, 0.1, 0.1 / 9, 1e-8
CASES = [((8, 8), 1 / 7, 1e-3), ((8, 8), 1 / 7, 1e-6), ((7, 5), 1 / 6, 1e-3), ((7, 5), 1 / 6, 1e-6)]
DOPRI5_COUNTS = {((8, 8), 1e-3): (17, 3), ((8, 8), 1e-6): (46, 2), ((7, 5), 1e-3): (13, 1), ((7, 5), 1e-6): (40, 2)}


def _case(grid, dx):
    return ar.heat_matrix(*grid, dx), np.random.default_rng(0).standard_normal(grid[0] * grid[1])


def test_symbols_are_declared_mirrored_and_exported():
    lib = _lib.get()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in ("mfx_rk_adaptive_workspace_bytes", "mfx_rk_solve_adaptive"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        decl = re.search(rf"\b{name}\s*\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name
    assert lib.mfx_version() == 201
    # struct mfx_rk_pair: the tableau, double e[16], int32 order; struct mfx_rk_adaptive_info: int32, 3 x int64, double
    P, I = _lib.RkPair, _lib.RkAdaptiveInfo
    tab = ctypes.sizeof(_lib.RkTableau)
    assert (P.tab.offset, P.e.offset, P.order.offset, ctypes.sizeof(P)) == (0, tab, tab + 128, tab + 136)
    assert (I.status.offset, I.n_accepted.offset, I.n_rejected.offset, I.n_attempts.offset, I.t_reached.offset, ctypes.sizeof(I)) == (0, 8, 16, 24, 32, 40)
    for name, value in (("MFX_RK_OK", 0), ("MFX_RK_MAX_ATTEMPTS", 1), ("MFX_RK_STEP_TOO_SMALL", 2), ("MFX_RK_NONFINITE", 3)):
        assert re.search(rf"\b{name} = {value}\b", header), name
    assert (_lib.RK_OK, _lib.RK_MAX_ATTEMPTS, _lib.RK_STEP_TOO_SMALL, _lib.RK_NONFINITE) == (ar.OK, ar.MAX_ATTEMPTS, ar.STEP_TOO_SMALL, ar.NONFINITE)


def test_pair_coefficients_are_scipys():
    from scipy.integrate._ivp.rk import RK23, RK45

    a, b, e = ar.full_pair(rk_tableaux.get_pair("dopri5"))
    assert np.array_equal(e, RK45.E) and np.array_equal(b[:6], RK45.B) and b[6] == 0.0
    assert np.array_equal(a[:6, :5], RK45.A) and np.array_equal(a[6, :6], RK45.B)  # the seventh stage is evaluated at y+
    assert rk_tableaux.get_pair("dopri5").order == RK45.error_estimator_order + 1 == 5
    assert rk_tableaux.get_pair("dopri5").tab is rk_tableaux.get("dopri5")
    a, b, e = ar.full_pair(rk_tableaux.get_pair("bosh3"))
    assert np.array_equal(e, RK23.E) and np.array_equal(b[:3], RK23.B) and b[3] == 0.0
    assert np.array_equal(a[:3, :3], RK23.A) and np.array_equal(a[3, :3], RK23.B)
    assert rk_tableaux.get_pair("bosh3").order == RK23.error_estimator_order + 1 == 3
    heun = rk_tableaux.get_pair("heun")
    assert heun.e == (-0.5, 0.5) and heun.order == 2 and heun.tab is rk_tableaux.get("heun")
    assert rk_tableaux.PAIR_NAMES == ("dopri5", "bosh3", "heun")
    with pytest.raises(NotImplementedError, match="dopri8"):
        rk_tableaux.get_pair("dopri8")
    with pytest.raises(ValueError, match="unknown"):
        rk_tableaux.get_pair("rk4")
    # the fixed-step names are what they were
    assert set(rk_tableaux.NAMES) == {"euler", "heun", "midpoint", "rk4", "dopri5", "dopri8"}
    st = rk_tableaux.pair_struct(rk_tableaux.get_pair("bosh3"))
    assert st.tab.stages == 4 and st.order == 3 and list(st.e)[:5] == [*RK23.E, 0.0] and st.tab.a[3][2] == RK23.B[2]


@pytest.mark.parametrize("method,name", [("RK45", "dopri5"), ("RK23", "bosh3")])
@pytest.mark.parametrize("grid,dx,rtol", CASES, ids=lambda v: str(v))
def test_restatement_takes_scipys_time_grid(grid, dx, rtol, method, name):
    from scipy.integrate import solve_ivp

    A, y0 = _case(grid, dx)
    res = ar.solve(A, y0, rk_tableaux.get_pair(name), T0, T1, DT0, rtol, ATOL)
    sol = solve_ivp(lambda t, y: A @ y, (T0, T1), y0, method=method, first_step=DT0, rtol=rtol, atol=ATOL)
    assert res["status"] == ar.OK and sol.status == 0
    assert len(sol.t) == len(res["ts"]), "the same number of accepted steps"
    stages = {"RK45": 6, "RK23": 3}[method]  # scipy: one evaluation up front, `stages` per attempt
    assert sol.nfev == 1 + stages * (res["n_accepted"] + res["n_rejected"]), "the same number of rejected steps"
    diff = float(np.abs(sol.t - res["ts"]).max())
    # RK45: 1.5e-14, measured 1.25e-14 at most.  RK23 takes up to 264 steps: a last-place difference in a norm moves every later grid
    # point, so the bound grows with the steps: 16 ulp(t1) per step
    bound = 1.5e-14 if method == "RK45" else max(1.5e-14, 16 * np.spacing(T1) * res["n_accepted"])
    print(f"{method} {grid} rtol {rtol}: {res['n_accepted']} + {res['n_rejected']} steps, grid differs by {diff:.3e} (bound {bound:.3e})")
    assert diff <= bound
    assert res["ts"][-1] == T1 and math.fsum(res["dts"]) == T1 - T0
    if name == "dopri5":
        assert (res["n_accepted"], res["n_rejected"]) == DOPRI5_COUNTS[(grid, rtol)]
        assert ar.clear_of_ties(res, 0.07), "every error norm stays 7 % away from 1"


def test_restatement_status_paths_and_fixed_step_blow_up():
    A, y0 = _case((8, 8), 1 / 7)
    pair = rk_tableaux.get_pair("dopri5")
    res = ar.solve(A, y0, pair, T0, T1, DT0, 1e-3, ATOL, max_attempts=5)
    assert res["status"] == ar.MAX_ATTEMPTS and res["n_accepted"] + res["n_rejected"] == 5 and res["ts"][-1] < T1
    assert ar.solve(A, y0, pair, 1.0, 1.1, 1e-16, 1e-3, ATOL)["status"] == ar.STEP_TOO_SMALL
    with np.errstate(all="ignore"):
        assert ar.solve(A, y0 * np.inf, pair, T0, T1, DT0, 1e-3, ATOL)["status"] == ar.NONFINITE
    # nine equal dopri5 steps are far outside the stability region: attempt() with no controller
    a, b, e = ar.full_pair(pair)
    y = y0[None]
    for _ in range(9):
        y, _ = ar.attempt(A, y, a, b, e, DT0, np.float64)
    assert 6e4 < np.abs(y).max() < 7e4
    import scipy.linalg

    exact = scipy.linalg.expm(T1 * A) @ y0
    assert 0.027 < np.abs(exact).max() < 0.029
    for rtol, err in ((1e-3, 6.4e-6), (1e-6, 8.9e-9)):
        got = np.abs(ar.solve(A, y0, pair, T0, T1, DT0, rtol, ATOL)["y1"][0] - exact).max()
        assert 0.9 * err < got < 1.1 * err, (rtol, got)


def _dense_desc(n=8):
    d = _lib.Operator()
    d.kind, d.dtype, d.n = _lib.OP_DENSE, _lib.MFX_F64, n
    d.dense_a, d.lda = 64, n
    return d


def _solve(lib, desc, pair, *, t0=0.0, t1=1.0, dt0=0.1, rtol=1e-3, atol=1e-6, max_steps=16, max_attempts=16, chunk=8, n=8, p=1, ld=None,
           ws_bytes=BIG, flags=0, info=True, y=FAKE):
    ld = n if ld is None else ld
    st = _lib.RkAdaptiveInfo()
    return lib.mfx_rk_solve_adaptive(ctypes.byref(desc), ctypes.byref(pair) if pair is not None else None, t0, t1, dt0, rtol, atol, max_steps,
                                     max_attempts, chunk, y, ld, n, p, FAKE, ld, None, None, ctypes.byref(st) if info else None, flags, FAKE,
                                     ws_bytes, None)


def test_refusals_come_before_any_launch():
    lib = _lib.get()
    desc = _dense_desc()
    err = lambda: lib.mfx_last_error().decode()  # noqa: E731

    def pair(**edit):
        q = rk_tableaux.pair_struct(rk_tableaux.get_pair("dopri5"))
        for key, v in edit.items():
            if key == "stages":
                q.tab.stages = v
            elif key == "a":
                q.tab.a[v[0]][v[1]] = v[2]
            elif key == "e":
                q.e[v[0]] = v[1]
            else:
                q.order = v
        return q

    good = pair()
    # everything the fixed-step drivers refuse
    for q in (pair(stages=0), pair(stages=17), pair(a=(1, 1, 0.5)), pair(a=(2, 1, float("nan")))):
        assert _solve(lib, desc, q) == -1 and "tableau" in err()
    broken = _dense_desc()
    broken.dense_a = None
    assert _solve(lib, broken, pair(stages=0)) == -1 and "dense operator without matrix" in err()
    rows = _dense_desc()
    rows.nrows = 4
    assert _solve(lib, rows, good) == -2 and "row-sharded" in err()
    assert _solve(lib, desc, good, p=0) == -1
    assert _solve(lib, desc, good, p=65536) == -2
    assert _solve(lib, desc, good, n=9) == -1
    assert _solve(lib, desc, good, ld=7) == -1 and "leading" in err()
    assert _solve(lib, desc, good, flags=2) == -1 and "flag" in err()
    # the entry's own
    assert _solve(lib, desc, None) == -1 and "pair is NULL" in err()
    assert _solve(lib, desc, pair(e=(3, float("nan")))) == -1 and "e[3]" in err()
    assert _solve(lib, desc, pair(e=(0, float("inf")))) == -1 and "e[0]" in err()
    for order in (0, -2):
        assert _solve(lib, desc, pair(order=order)) == -1 and "order" in err()
    for rtol, atol in ((0.0, 0.0), (-1e-3, 1.0), (1e-3, -1e-9), (float("nan"), 1e-6), (1e-3, float("inf"))):
        assert _solve(lib, desc, good, rtol=rtol, atol=atol) == -1 and "rtol" in err(), (rtol, atol)
    for dt0 in (0.0, -0.1, float("nan")):
        assert _solve(lib, desc, good, dt0=dt0) == -1 and ("dt0" in err() or "dts" in err())
    for t0, t1 in ((0.0, 0.0), (1.0, 0.5), (0.0, float("inf")), (float("nan"), 1.0)):
        assert _solve(lib, desc, good, t0=t0, t1=t1) == -1 and "t1" in err()
    assert _solve(lib, desc, good, max_steps=0) == -1 and "max_steps" in err()
    assert _solve(lib, desc, good, max_attempts=0) == -1 and "max_attempts" in err()
    assert _solve(lib, desc, good, chunk=0) == -1 and "chunk" in err()
    assert _solve(lib, desc, good, info=False) == -1 and "null" in err()
    assert _solve(lib, desc, good, y=None) == -1 and "null" in err()
    # the workspace: exact, refused when short
    need = lib.mfx_rk_adaptive_workspace_bytes(ctypes.byref(desc), ctypes.byref(good), 8, 1, 16)
    assert need > 0 and need % 256 == 0
    assert _solve(lib, desc, good, ws_bytes=need - 1) == -4 and "workspace" in err()
    assert _solve(lib, desc, good, ws_bytes=255) == -4


def test_workspace_query_is_monotone_and_refuses():
    lib = _lib.get()
    good = rk_tableaux.pair_struct(rk_tableaux.get_pair("dopri5"))
    small = rk_tableaux.pair_struct(rk_tableaux.get_pair("heun"))
    n = 1027
    desc = _dense_desc(n)
    q = lambda pr, p, m, nn=n, d=desc: lib.mfx_rk_adaptive_workspace_bytes(ctypes.byref(d), ctypes.byref(pr), nn, p, m)  # noqa: E731
    by_p = [q(good, p, 64) for p in (1, 2, 3, 7, 64)]
    by_m = [q(good, 3, m) for m in (1, 31, 32, 33, 4096, 1 << 20)]
    assert all(a < b for a, b in zip(by_p, by_p[1:])) and by_p[0] > 0
    assert all(a <= b for a, b in zip(by_m, by_m[1:])) and by_m[0] < by_m[-1] and by_m[-1] - by_m[0] >= 8 * ((1 << 20) - 32)
    assert q(small, 3, 64) < q(good, 3, 64)
    # the vectors alone: y, y+, the stage value and seven K rows of p n doubles
    assert by_p[2] >= 10 * 3 * n * 8
    for args in ((good, 0, 64), (good, 3, 0), (good, 3, 64, n + 1)):
        assert q(*args) == -1
    bad = rk_tableaux.pair_struct(rk_tableaux.get_pair("dopri5"))
    bad.tab.stages = 17
    assert q(bad, 3, 64) == -1
    assert lib.mfx_rk_adaptive_workspace_bytes(None, ctypes.byref(good), n, 1, 8) == -1
    assert lib.mfx_rk_adaptive_workspace_bytes(ctypes.byref(desc), None, n, 1, 8) == -1


def test_python_layer_refusals():
    kw = dict(rtol=1e-3, atol=1e-6)
    with pytest.raises(TypeError, match="linear operator"):
        pde_util.solver_rk_adaptive(0.0, 1.0, lambda v: v, **kw)
    with pytest.raises(NotImplementedError, match="dopri8"):
        pde_util.solver_rk_adaptive(0.0, 1.0, DenseOp(), method="dopri8", **kw)
    with pytest.raises(ValueError, match="unknown"):
        pde_util.solver_rk_adaptive(0.0, 1.0, DenseOp(), method="rk4", **kw)
    with pytest.raises(ValueError, match="adjoint"):
        pde_util.solver_rk_adaptive(0.0, 1.0, DenseOp(), adjoint="forward", **kw)
    with pytest.raises(ValueError, match="t1"):
        pde_util.solver_rk_adaptive(1.0, 1.0, DenseOp(), **kw)
    with pytest.raises(ValueError, match="max_steps"):
        pde_util.solver_rk_adaptive(0.0, 1.0, DenseOp(), max_steps=0, **kw)
    with pytest.raises(TypeError):
        pde_util.solver_rk_adaptive(0.0, 1.0, DenseOp())  # rtol and atol have no default
    sharded = RowShardedOp.__new__(RowShardedOp)
    sharded.op, sharded.comm, sharded.plans = DenseOp(), None, None
    with pytest.raises(NotImplementedError, match="row-sharded"):
        pde_util.solver_rk_adaptive(0.0, 1.0, sharded, **kw)
    for name in ("recursive_checkpoint", "direct", "backsolve", "discrete"):
        pde_util.solver_rk_adaptive(0.0, 1.0, DenseOp(), adjoint=name, **kw)
    solve = pde_util.solver_rk_adaptive(0.0, 1.0, DenseOp(), dt0=0.1, **kw)
    with pytest.raises(_lib.MfxError, match="ROCm device"):
        solve(torch.ones(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64))
    assert "not differentiated" in pde_util.solver_rk_adaptive.__doc__.lower() or "NOT differentiated" in pde_util.solver_rk_adaptive.__doc__
