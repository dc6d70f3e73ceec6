"""CPU checks of tests/_ragged_csr.py: the generator keeps its promises (every row length, longest row and column, empty runs, no
duplicates), the Krylov cases of tests/test_gpu_operator_kernels.py stay clear of breakdown in the fp64 oracle, and their (n, p)
reach every launch geometry of the fused CSR step."""

import numpy as np
import pytest

import _ragged_csr as rc
from oracle import slq_oracle as orc


def _default(n=1000, seed=0, **kw):
    return rc.ragged_csr(n, np.random.default_rng(seed), **kw)


def test_offsets_are_distinct_modulo_every_admissible_n():
    for L in range(1, 65):
        for n in (L, L + 1, 2 * L + 1, 1000):
            assert len({o % n for o in rc.OFFSETS[:L]}) == L, (L, n)


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 1000, 1531])
def test_no_duplicates_rows_sorted_and_forced_rows_empty(n):
    runs = ((5, 20),) if n >= 31 else ()
    row, col, vals = _default(n, seed=n, empty_runs=runs)
    assert len(np.unique(row * n + col)) == len(row)
    assert (np.diff(row) >= 0).all() and ((0 <= col) & (col < n)).all()
    rows, cols = rc.row_and_col_lengths(row, col, n)
    assert (rows[rc.empty_rows(n, runs)] == 0).all()
    assert rows.max(initial=0) <= min(n, 64) and cols.max(initial=0) <= min(n, 64)
    assert np.array_equal(vals[row == col] > 1.5, np.ones((row == col).sum(), dtype=bool))  # 3 + 0.3 N(0, 1) on the diagonal


def test_every_length_occurs_and_the_longest_row_and_column_are_64():
    row, col, _ = _default(1000)
    rows, cols = rc.row_and_col_lengths(row, col, 1000)
    assert set(rc.DEFAULT_LENGTHS) <= set(rows.tolist())
    assert rows.max() == 64 and cols.max() == 64
    assert cols[rc.full_column(1000)] == 64
    _, cols_run = rc.row_and_col_lengths(*_default(1000, empty_runs=((100, 100),))[:2], 1000)
    assert (cols_run[140:160] == 0).all()  # empty columns inside a long empty run: rows of A^T with nothing to gather
    assert not np.array_equal(rows, cols)  # non-symmetric pattern: the transposed structure is another matrix


def test_the_65_case_has_one_row_and_one_column_of_65():
    n = 1536
    row, col, vals = rc.krylov_switch_case(65)
    rows, cols = rc.row_and_col_lengths(row, col, n)
    assert rows.max() == 65 and cols.max() == 65 and (rows == 65).sum() == 1 and (cols == 65).sum() == 1
    assert len(np.unique(row * n + col)) == len(row)
    row, col, vals = rc.krylov_switch_case(64)
    rows, cols = rc.row_and_col_lengths(row, col, n)
    assert rows.max() == 64 and cols.max() == 64


def test_the_mean_rule_case_has_a_short_mean_and_one_row_of_200():
    n = 1536
    row, col, vals = rc.krylov_switch_case(200)
    rows, _ = rc.row_and_col_lengths(row, col, n)
    assert rows.max() == 200 and (rows > 64).sum() == 1
    assert len(row) <= 24 * n  # csr_fusable's mean rule keeps the fused step when max_row_nnz is not stated
    assert len(np.unique(row * n + col)) == len(row)


@pytest.mark.parametrize("case", rc.KRYLOV_CASES, ids=[c[0] for c in rc.KRYLOV_CASES])
def test_empty_runs_of_the_krylov_cases_are_empty(case):
    name, n, p, run, _ = case
    row, col, vals, V = rc.krylov_case(name)
    rows, _ = rc.row_and_col_lengths(row, col, n)
    assert (rows[run[0] : run[0] + run[1]] == 0).all() and rows[0] == 0 and rows[-1] == 0
    assert rows.max() == 64 and V.shape == (p, n)


def _margins(o, k, v, vals, reortho):
    _, H, r, _ = orc.arnoldi_forward(o, k, v, vals, reortho=reortho)
    scale = np.abs(H).max()
    return np.concatenate([np.diag(H, -1), [np.linalg.norm(r)]]) / scale


def _assert_no_near_breakdown(row, col, vals, n, probes, what):
    o = orc.CooOp(row, col, n)
    for k in rc.KRYLOV_DEPTHS:
        for reortho in ("full", "none"):
            for b, v in probes:
                m = _margins(o, k, v, vals, reortho)
                assert m.min() >= 1e-3, (what, k, reortho, b, m.min())


@pytest.mark.parametrize("case", rc.KRYLOV_CASES, ids=[c[0] for c in rc.KRYLOV_CASES])
def test_krylov_cases_stay_clear_of_breakdown(case):
    """every subdiagonal H[i+1, i] and |r| at least 1e-3 max|H|, for every depth, both reortho modes and every probe the GPU test
    compares with the oracle: the GPU comparison at 1e-9 is then a parity test, not a race between two chaotic recurrences"""
    name, n, p, _, _ = case
    row, col, vals, V = rc.krylov_case(name)
    _assert_no_near_breakdown(row, col, vals, n, [(b, V[b]) for b in rc.oracle_probes(p)], name)


def test_the_unsampled_probes_of_the_wide_cases_stay_clear_of_breakdown():
    """the fp32-against-fp64 comparison covers all probes of the 64- and 128-vector cases: their margins at the deepest recurrence
    (the shallower ones are its leading blocks)"""
    for name, n, p, _, _ in rc.KRYLOV_CASES:
        if p <= 16:
            continue
        row, col, vals, V = rc.krylov_case(name)
        o = orc.CooOp(row, col, n)
        for b in range(p):
            assert _margins(o, max(rc.KRYLOV_DEPTHS), V[b], vals, "full").min() >= 1e-3, (name, b)


@pytest.mark.parametrize("longest", [64, 65, 200])
def test_switch_cases_stay_clear_of_breakdown(longest):
    row, col, vals = rc.krylov_switch_case(longest)
    _assert_no_near_breakdown(row, col, vals, 1536, [(0, rc.krylov_switch_vector())], longest)


def test_three_term_recurrence_of_the_krylov_cases_has_no_small_offdiagonal():
    """lanczos.tridiag(reortho="none") forward runs on the same matrices: its b_i against max(|a|, |b|)"""
    for name, n, p, _, _ in rc.KRYLOV_CASES:
        row, col, vals, V = rc.krylov_case(name)
        o = orc.CooOp(row, col, n)
        for b in rc.oracle_probes(p):
            (_, (a, off)), (_, last) = orc.tridiag(o, min(max(rc.KRYLOV_DEPTHS), 8), V[b], vals, reortho="none")
            assert min(np.abs(off).min(), abs(last)) >= 1e-3 * max(np.abs(a).max(), np.abs(off).max()), (name, b)


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_geometry_rules(dtype_name):
    w = rc.VEC_WIDTH[dtype_name]
    g = lambda n, p, **kw: rc.csr_step_geometry(n, p, dtype_name, **kw)  # noqa: E731
    assert g(1531, 1) == (64, 1, 8) and g(1536, 1) == (64, w, 8)
    assert g(1536, 1, aligned=False) == (64, 1, 8)
    assert g(1027, 16) == (256, 1, 8) and g(1028, 16) == (256, w, w) and g(1028, 128) == (256, w, 8)
    assert g(1028, 15) == (64, w, 8)  # 1 slice x 15 vectors < 16: one wave
    assert g(2049, 8) == (256, 1, 8) and g(2048, 8) == (64, w, 8)  # pick_wg counts 2048-element slices
    assert g(1028, 127) == (256, w, w) and g(2052, 64) == (256, w, 8)  # fine only below 128 workgroups


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_the_krylov_cases_cover_every_geometry_of_the_fused_step(dtype_name):
    table = [rc.csr_step_geometry(n, p, dtype_name) for _, n, p, _, _ in rc.TABLE_CASES]
    assert len(set(table)) == 5 and set(table) == rc.all_geometries(dtype_name)
    w = rc.VEC_WIDTH[dtype_name]
    assert table == [(64, 1, 8), (64, w, 8), (256, 1, 8), (256, w, w), (256, w, 8)]  # in the order of the case names
    assert {rc.csr_step_geometry(n, p, dtype_name) for _, n, p, _, _ in rc.KRYLOV_CASES} == rc.all_geometries(dtype_name)


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_empty_runs_cover_a_whole_workgroup_where_n_has_a_second_slice(dtype_name):
    for name, n, p, (start, count), _ in rc.KRYLOV_CASES:
        wg, _, ept = rc.csr_step_geometry(n, p, dtype_name)
        sl = wg * ept
        whole = [s for s in range(-(-n // sl)) if start <= s * sl and min((s + 1) * sl, n) <= start + count]
        if name in ("wg256-scalar", "wg256-coarse") or (name == "wg256-fine" and dtype_name == "float32"):
            assert n <= sl + 4 and not whole  # one slice holds (all but 4 rows of) the matrix: nothing to empty without emptying it
        else:
            assert whole, (name, dtype_name)


def test_bounds_are_the_stated_formulas():
    u = rc.unit_roundoff("float32")
    assert rc.apply_bound(np.array([0, 5]), u, np.array([0.0, 2.0])).tolist() == [0.0, 2 * 13 * u * 2.0]
    assert rc.grad_bound(7, u, 2.0, -3.0) == (14 * 2.0**-53 + 2 * u) * 2.0 + 3 * u


def test_references_against_the_coo_oracle():
    n = 33
    row, col, vals = _default(n, seed=3)
    A, o = rc.dense_of(row, col, vals, n), orc.CooOp(row, col, n)
    X = np.random.default_rng(4).standard_normal((2, n))
    assert np.allclose(rc.apply_ref(A, X)[0], np.stack([o.apply(x, vals) for x in X]), rtol=1e-13, atol=1e-13)
    assert np.allclose(rc.apply_ref(A, X, True)[0], np.stack([o.apply_t(x, vals) for x in X]), rtol=1e-13, atol=1e-13)
    assert np.allclose(rc.outer_ref(X, X[::-1])[0][row, col], o.param_vjp(X[::-1], X, vals)[0], rtol=1e-13, atol=1e-13)
