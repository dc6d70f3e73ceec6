"""tests/_cg_cases.py against itself and the oracle, on the CPU: the launch geometry every case line claims, the restated
adaptive loop, partial Cholesky and Woodbury solve against oracle/slq_oracle.py in float64, the margins that make the number of
adaptive steps and the pivots independent of rounding, and the error bounds against a fresh measurement of the oracle's own
rounding error (longdouble as the yardstick)."""

import numpy as np
import pytest

import _cg_cases as cc
import _ragged_csr as rc
from oracle import slq_oracle as orc

DTYPES = ("float32", "float64")


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", cc.SOLVE_NAMES)
def test_every_case_reaches_the_branches_its_line_names(name, dtype_name):
    _, n, p, rank, steps, _, claims = cc.solve_case(name)
    assert claims and 1 <= steps <= 8
    for token in claims:
        assert cc.claim_holds(token, n, p, rank, dtype_name), (name, token, cc.cg_geometry(n, p, dtype_name))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_cases_together_cover_every_geometry_and_rank_path(dtype_name):
    w = rc.VEC_WIDTH[dtype_name]
    geo = [cc.cg_geometry(n, p, dtype_name) for _, n, p, _, _, _, _ in cc.SOLVE_CASES]
    assert {g[:2] for g in geo} == {(64, 1), (64, w), (256, 1), (256, w)}
    nblk = [g[2] for g in geo]
    assert any(b == 1 for b in nblk) and any(1 < b <= 64 for b in nblk) and any(64 < b <= 512 for b in nblk) and any(b > 512 for b in nblk)
    ranks = {c[3] for c in cc.SOLVE_CASES}
    assert {1, 3, 4, 5, 257, 1024} <= ranks
    assert {c[3] for c in cc.SOLVE_CASES if c[0] in cc.APPLY_NAMES} >= {1, 3, 4, 5, 257, 1024}
    assert all(c[1] >= 1027 for c in cc.SOLVE_CASES if c[3] == 257)
    # the 1050628 case is kept: 514 slices is the only count at which the loop of reduce_partials_group<T, 64> runs twice
    assert cc.cg_geometry(133121, 1, dtype_name)[2] == 66 and cc.cg_geometry(1050628, 1, dtype_name)[2] == 514
    # large cases stay cheap
    assert all(p == 1 and steps <= 4 and rank <= 5 for _, n, p, rank, steps, _, _ in cc.SOLVE_CASES if n > 100000)


def test_the_issue_table_of_geometries():
    g = cc.cg_geometry
    assert g(1531, 1, "float32") == g(1531, 1, "float64") == (64, 1, 3)
    assert g(1536, 1, "float32") == (64, 4, 3) and g(1536, 1, "float64") == (64, 2, 3)
    assert g(1027, 16, "float32") == (256, 1, 1) and g(1028, 16, "float32") == (256, 4, 1) and g(1028, 16, "float64") == (256, 2, 1)
    assert g(3075, 16, "float64") == (256, 1, 2) and g(3076, 16, "float32") == (256, 4, 2)
    assert g(133121, 1, "float32") == (256, 1, 66) and g(133124, 1, "float64") == (256, 2, 66)
    assert g(1028, 1, "float32", aligned=False) == (64, 1, 3)
    # the adaptive batch and its columns alone, and the re-orthogonalising cases: one geometry, so the same bits
    assert g(cc.ADAPTIVE_N, 3, "float32") == g(cc.ADAPTIVE_N, 1, "float32") == (64, 4, 2)
    assert g(cc.ADAPTIVE_N, 3, "float64") == g(cc.ADAPTIVE_N, 1, "float64") == g(cc.ADAPTIVE_N, 2, "float64") == (64, 2, 2)
    ids = {cc.solve_id(name) for name in cc.SOLVE_NAMES}
    assert len(ids) == len(cc.SOLVE_NAMES)
    assert cc.solve_id("wg256-vector") == "wg256-vector-n1028-p16-rank5-steps4-f32:wg256.vec4.nblk1-f64:wg256.vec2.nblk1"


def test_reortho_cases_put_the_rank_on_either_side_of_the_depth():
    sides = {(rank > m) - (rank < m) for _, _, _, rank, m in cc.REORTHO_CASES if rank}
    assert sides == {-1, 1} and any(rank == 0 for _, _, _, rank, _ in cc.REORTHO_CASES)
    for _, n, p, _, m in cc.REORTHO_CASES:
        assert cc.cg_geometry(n, p, "float32")[2] == 2 and 1 <= m <= 8


def test_cholesky_sizes_straddle_the_256_row_blocks():
    sizes = {c[1] for c in cc.CHOL_CASES}
    assert {255, 256, 257, 65537} <= sizes and -(-65537 // 256) == 257
    for kind in ("dense", "gram"):
        assert {c[4] for c in cc.CHOL_CASES if c[3] == kind} == {0, 1}
    assert {c[5] for c in cc.CHOL_CASES if c[3] == "gram"} == {0, 1}


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _is_f32(a):
    return (np.asarray(a, dtype=np.float32).astype(np.float64) == a).all()


@pytest.mark.parametrize("name", ["one-wave-scalar", "wg256-scalar", "many-slices-scalar"])
def test_inputs_are_float32_values_and_the_preconditioner_is_symmetric_positive_definite(name):
    s = cc.solve_inputs(name)
    assert s.Lt.shape == (s.rank, s.n) and s.minv.shape == (s.rank, s.rank)
    assert _is_f32(s.Lt) and _is_f32(s.minv) and _is_f32(s.B) and _is_f32(s.V)
    assert (s.minv == s.minv.T).all() and np.linalg.eigvalsh(s.minv).min() > 0.0
    if s.kind == "dense":
        assert _is_f32(s.A) and (s.A == s.A.T).all()
        w = np.linalg.eigvalsh(s.A)
        assert 0.99 < w.min() and w.max() < 10.01
        # the factor is the pivoted partial Cholesky factor: A - L L^T is positive semi-definite and zero on the pivots
        res = s.A - s.Lt.T @ s.Lt
        assert np.linalg.eigvalsh(res).min() > -1e-5 and np.sort(np.abs(np.diagonal(res)))[: s.rank].max() < 1e-5
    # minv is the inverse of s I + L^T L up to its rounding to float32
    cap = cc.SHIFT * np.eye(s.rank) + s.Lt @ s.Lt.T
    assert np.abs(s.minv @ cap - np.eye(s.rank)).max() < 1e-4


# ------------------------------------------------------------------------------------------------
# the restatements against the oracle, float64
# ------------------------------------------------------------------------------------------------
def test_adaptive_trace_is_the_oracle_loop():
    s = cc.adaptive_inputs()
    A, P = cc.matvec(s, np.float64), cc.preconditioner(s, np.float64)
    for b in range(s.p):
        kw = dict(atol=cc.ADAPTIVE_ATOL, rtol=cc.ADAPTIVE_RTOL, maxiter=cc.ADAPTIVE_MAXITER)
        x, r, nsteps, measures = cc.pcg_adaptive_trace(A, s.B[b], P, **kw)
        x_ref, info = orc.pcg_adaptive(A, s.B[b], P, **kw)
        assert (x == x_ref).all() and (r == info["residual_abs"]).all() and nsteps == info["num_steps"]
        assert len(measures) == nsteps + 1


@pytest.mark.parametrize("name", ["dense-255-pivot", "gram-255-pivot", "dense-257-plain", "gram-257-plain"])
def test_columnwise_cholesky_is_the_oracle_factor(name):
    s = cc.chol_inputs(name)
    column, diagonal = cc.chol_columns(s, np.float64)
    L, pivots, success, _ = cc.cholesky_partial(column, diagonal, s.n, s.rank, np.float64, bool(s.pivot))
    cols = {}

    def element(i, j):
        if j not in cols:
            cols[j] = column(j)
        return cols[j][i]

    if s.pivot:
        L_ref, info = orc.cholesky_partial_pivot(element, s.n, s.rank)
        assert (pivots == info["pivots"]).all() and success == info["success"]
    else:
        L_ref, _ = orc.cholesky_partial(element, s.n, s.rank)
        assert (pivots == np.arange(s.rank)).all() and success
    assert np.abs(L - L_ref).max() <= 1e-13 * np.abs(L_ref).max()


def test_woodbury_with_the_exact_minv_is_the_oracle_solve():
    s = cc.solve_inputs("wg256-vector")
    minv = np.linalg.inv(cc.SHIFT * np.eye(s.rank) + s.Lt @ s.Lt.T)
    for v in s.V[:3]:
        z = cc.woodbury_apply(s.Lt, minv, cc.SHIFT, v)
        z_ref = orc.precondition_solve(s.Lt.T.copy(), v, cc.SHIFT)
        assert np.abs(z - z_ref).max() <= 1e-13 * np.abs(z_ref).max()
        # and rounding minv to float32 moves it by about 2^-24, far more than the float64 bounds: why the reference keeps it
        assert np.abs(cc.woodbury_apply(s.Lt, s.minv, cc.SHIFT, v) - z_ref).max() > 1e-12 * np.abs(z_ref).max()


@pytest.mark.parametrize("dtype_name", ["float32", "longdouble"])
def test_every_wrapper_keeps_the_float_type(dtype_name):
    dtype = np.dtype(dtype_name).type
    for key in ("solve/wg256-vector/pre", "adaptive", "reortho/rank-below", "apply/wg256-vector", "chol/gram-257-pivot"):
        out = cc.run(key, dtype_name)
        assert all(out[o].dtype == dtype for o in cc.outputs_of(key)), key


# ------------------------------------------------------------------------------------------------
# margins: what makes the step counts and the pivots the same in every float type
# ------------------------------------------------------------------------------------------------
def test_no_stopping_measure_of_the_adaptive_batch_is_near_one():
    out = cc.run("adaptive")
    assert sorted(out["num_steps"].tolist()) == [1, 2, 4] and out["num_steps"].max() < cc.ADAPTIVE_MAXITER
    for b, measures in enumerate(out["measures"]):
        m = np.asarray(measures, dtype=np.float64)
        print(f"column {b}: {out['num_steps'][b]} steps, measures {np.array2string(m, precision=3)}")
        assert ((m < 0.5) | (m > 2.0)).all(), (b, m)
    for dt in DTYPES:  # hence the oracle itself stops at the same steps in both types
        assert (cc.run("adaptive", dt)["num_steps"] == out["num_steps"]).all()


@pytest.mark.parametrize("name", [c[0] for c in cc.CHOL_CASES if c[4]])
def test_every_pivot_wins_by_a_relative_margin_or_by_an_exact_tie(name):
    """winner >= (1 + 1e-3) runner-up at every step -- except step 0 of a Gram operator, where all n diagonal entries are one and
    the same number in every float type (the distance of a point to itself is exactly 0): an exact tie, which row 0 wins"""
    s = cc.chol_inputs(name)
    out = cc.run(f"chol/{name}")
    assert tuple(out["pivots"]) == cc.expected_pivots(name) and out["success"]
    for i, (win, second) in enumerate(out["margins"]):
        if s.kind == "gram" and i == 0:
            assert win == second and out["pivots"][0] == 0
            for dt in DTYPES:
                assert len(set(cc.chol_columns(s, np.dtype(dt).type)[1]().tolist())) == 1
        else:
            assert win - second >= 1e-3 * win, (name, i, win, second)
    for dt in DTYPES:
        assert (cc.run(f"chol/{name}", dt)["pivots"] == out["pivots"]).all()


def test_the_first_pivot_of_the_largest_case_sits_behind_256_blocks():
    assert cc.run("chol/gram-65537-pivot")["pivots"][1] // 256 == 256  # the second trip of a thread's loop over the block winners


def test_exact_ties_go_to_the_first_index_in_the_oracle_too():
    A = cc.tie_matrix()
    assert (A == A.T).all() and (A == np.round(A)).all() and np.linalg.eigvalsh(A).min() > 0
    assert len({p // 256 for p in cc.TIE_PIVOTS[:3]}) == 3
    L_ref, info = orc.cholesky_partial_pivot(lambda i, j: A[i, j], len(A), len(cc.TIE_PIVOTS))
    assert tuple(info["pivots"]) == cc.TIE_PIVOTS and info["success"]
    for dtype in (np.float32, np.longdouble):
        col, diag = cc.dense_columns(A.astype(dtype))
        L, pivots, success, margins = cc.cholesky_partial(col, diag, len(A), len(cc.TIE_PIVOTS), dtype, True)
        assert tuple(pivots) == cc.TIE_PIVOTS and success
        assert (L.astype(np.float64) == L_ref).all()  # exact arithmetic
        assert [win == second for win, second in margins] == [True, True, False, True]


def test_rank_deficient_matrix_fails_at_step_one():
    A, v = cc.deficient_matrix()
    assert np.linalg.matrix_rank(A) == 1 and (A == np.round(A)).all()
    for dtype in (np.float32, np.float64):
        col, diag = cc.dense_columns(A.astype(dtype))
        L, pivots, success, _ = cc.cholesky_partial(col, diag, len(A), 3, dtype, False)
        assert not success and (L[:, 0] == v).all() and np.isnan(L[:, 1:]).all() and tuple(pivots) == (0, 1, 2)
        Lp, pivots, success, _ = cc.cholesky_partial(col, diag, len(A), 2, dtype, True)
        assert not success and pivots[0] == 5 and (Lp[:, 0] == v).all()
    _, info = orc.cholesky_partial_pivot(lambda i, j: A[i, j], len(A), 2)
    assert info["success"] is False


# ------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------
def test_the_table_has_a_bound_for_every_output_of_every_key():
    assert set(cc.BOUNDS) == set(cc.keys())
    for key in cc.keys():
        for dt in cc.DTYPES:
            assert set(cc.bounds(key, dt)) == set(cc.outputs_of(key)), (key, dt)


@pytest.mark.parametrize("key", cc.keys())
def test_stored_bounds_are_32_times_the_measured_oracle_error(key):
    """each stored bound within [16, 64] x the freshly measured e64 / e32; hard caps as conditions"""
    measured = cc.measure(key)
    for dt, cap in (("float64", cc.FP64_CAP), ("float32", cc.FP32_CAP)):
        stored = cc.bounds(key, dt)
        for o in cc.outputs_of(key):
            e = measured[dt][o]
            print(f"{key} {dt} {o}: e = {e:.3e}, bound = {stored[o]:.3e}")
            assert 16.0 * e <= stored[o] <= 64.0 * e, (key, dt, o, e, stored[o])
            assert stored[o] <= cap, (key, dt, o, stored[o])
