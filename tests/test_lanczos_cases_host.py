"""tests/_lanczos_cases.py against itself and the oracle, on the CPU: the launch geometries the cases claim to reach, the
no-breakdown margins, the step-wise adjoint reference against orc.tridiag_none_vjp, and the error bounds against a fresh
measurement of the oracle's own rounding error (longdouble as the yardstick)."""

import numpy as np
import pytest

import _lanczos_cases as lc
import _ragged_csr as rc
from oracle import slq_oracle as orc

DTYPES = ("float32", "float64")


def test_case_ids_state_the_geometry_of_both_drivers_in_both_types():
    ident = lc.geometry_id("wg256-vector")
    assert ident == ("wg256-vector-n1028-p16-k4-f32fwd:wg256.vec4.ept4.nblk2-f32adj:wg256.vec4.ept8.nblk1"
                     "-f64fwd:wg256.vec2.ept2.nblk3-f64adj:wg256.vec2.ept8.nblk1")
    assert len({lc.geometry_id(name) for name in lc.NAMES}) == len(lc.NAMES)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_cases_reach_every_geometry(dtype_name):
    """every (wg, VEC, EPT) of the forward, every (wg, VEC) of the adjoint (EPT always 8), the misaligned scalar fallback of the
    adjoint variants, and the slice counts at which reduce_partials_group<T, 64> changes its path: (64, 512] and above 512"""
    fwd = {lc.lanczos_geometry(n, p, dtype_name)[:3] for _, n, p, _, _ in lc.CASES}
    assert fwd == rc.all_geometries(dtype_name)
    adj = [lc.lanczos_geometry(n, p, dtype_name, adjoint=True) for _, n, p, _, _ in lc.CASES]
    w = rc.VEC_WIDTH[dtype_name]
    assert {g[:3] for g in adj} == {(64, 1, 8), (64, w, 8), (256, 1, 8), (256, w, 8)}
    for geometries in (adj, [lc.lanczos_geometry(n, p, dtype_name) for _, n, p, _, _ in lc.CASES]):
        nblk = [g[3] for g in geometries]
        assert any(64 < b <= 512 for b in nblk) and any(b > 512 for b in nblk) and any(b == 1 for b in nblk)
        assert any(g[0] == 256 and 1 < g[3] <= 64 for g in geometries)  # more than one 2048-element slice, one load slot
    for name in lc.ADJOINT_VARIANT_CASES:  # a pointer 4 / 8 bytes into its allocation: scalar loads, same slicing
        _, n, p, _, _ = lc.case(name)
        aligned = lc.lanczos_geometry(n, p, dtype_name, adjoint=True)
        wg, vec, ept, nblk = lc.lanczos_geometry(n, p, dtype_name, aligned=False, adjoint=True)
        assert vec == 1 and (wg, ept, nblk) == (aligned[0], aligned[2], aligned[3])
        assert (aligned[1] > 1) == (n % w == 0)


def test_the_issue_table_of_geometries():
    g = lc.lanczos_geometry
    assert g(1531, 1, "float32") == (64, 1, 8, 3) and g(1531, 1, "float64", adjoint=True) == (64, 1, 8, 3)
    assert g(1536, 1, "float32") == (64, 4, 8, 3) and g(1536, 1, "float64") == (64, 2, 8, 3)
    assert g(1027, 16, "float32") == (256, 1, 8, 1)
    assert g(1028, 16, "float32") == (256, 4, 4, 2) and g(1028, 16, "float64") == (256, 2, 2, 3)
    assert g(1028, 16, "float64", adjoint=True) == (256, 2, 8, 1)
    assert g(1028, 128, "float32") == (256, 4, 8, 1) and g(1028, 128, "float64") == (256, 2, 8, 1)
    assert g(3075, 16, "float64") == (256, 1, 8, 2) and g(3076, 16, "float32", adjoint=True) == (256, 4, 8, 2)
    assert g(133121, 1, "float32", adjoint=True) == (256, 1, 8, 66)
    assert g(133124, 1, "float64") == (256, 2, 2, 261) and g(133124, 1, "float32") == (256, 4, 4, 131)
    assert g(133124, 1, "float64", adjoint=True) == (256, 2, 8, 66)
    assert g(1050628, 1, "float32") == g(1050628, 1, "float32", adjoint=True) == (256, 4, 8, 514)


def test_fused_step_follows_csr_fusable():
    """csr_fusable looks at the operator alone: the sparse cases (longest row 5) take the fused step at every slicing, the
    dense ones never do -- they run launch_dots, the single k_update and launch_scale of the unfused recurrence"""
    for name in lc.NAMES:
        assert lc.takes_fused_csr_step(name) == (lc.case(name)[4] == "sparse")
    s = lc.case_inputs("many-slices-scalar")
    assert np.bincount(s.row).max() == 5 and np.bincount(s.col).max() == 5


@pytest.mark.parametrize("name", lc.NAMES)
def test_operators_are_symmetric_and_no_case_breaks_down(name):
    """every beta_j of every probe is at least 1e-2 of the largest tridiagonal entry: k <= 9 steps lose no orthogonality, and a
    rounding-sized change of the input cannot move the outputs by more than the bounds allow"""
    s = lc.case_inputs(name)
    if s.kind == "dense":
        assert (s.A == s.A.T).all()
    else:
        fwd, bwd = np.lexsort((s.col, s.row)), np.lexsort((s.row, s.col))
        assert (s.row[fwd] == s.col[bwd]).all() and (s.col[fwd] == s.row[bwd]).all() and (s.vals[fwd] == s.vals[bwd]).all()
    xs, alpha, beta = lc.forward_pass(name, np.float64)
    scale = np.maximum(np.abs(alpha).max(axis=1), np.abs(beta).max(axis=1))
    assert (beta.min(axis=1) >= 1e-2 * scale).all(), (beta.min(), scale.max())
    for b in range(0, s.p, max(1, s.p // 4)):
        gram = xs[b] @ xs[b].T
        assert np.abs(gram - np.eye(s.k + 1)).max() < 1e-10


@pytest.mark.parametrize("name", ["one-wave-scalar", "depth-one", "wg256-vector", "many-slices-scalar"])
def test_stepwise_adjoint_agrees_with_the_oracle(name):
    s = lc.case_inputs(name)
    dense_all_rows = s.kind == "dense"
    op, params = (orc.DenseOp(), (s.A,)) if dense_all_rows else lc.oracle_operator(s, np.float64)
    for b in lc.reference_probes(name)[:2]:
        cot = lc.cotangent(s.dxs[b], s.dalpha[b], s.dbeta[b])
        dv_ref, (dp_ref,) = orc.tridiag_none_vjp(op, s.k, s.V[b], params, cot)
        dv, (dp,), lams, munu = lc.tridiag_none_vjp_states(op, s.k, s.V[b], params, cot)
        assert np.abs(dv - dv_ref).max() <= 1e-13 * np.abs(dv_ref).max()
        assert np.abs(dp - dp_ref).max() <= 1e-13 * np.abs(dp_ref).max()
        assert lams.shape == (s.k, s.n) and munu.shape == (s.k, 2)
        # the states are what the gradient contracts: sum_j x_j lambda_j^T
        (xs, _), _ = orc.tridiag_none(op, s.k, s.V[b], *params)
        (dp_states,) = op.param_vjp(lams, xs, *params)
        assert np.abs(dp_states - dp_ref).max() <= 1e-13 * np.abs(dp_ref).max()
        # a forward pass handed in gives the same as the oracle's own
        fwd = lc.forward_pass(name, np.float64, [b])
        again = lc.tridiag_none_vjp_states(op, s.k, s.V[b], params, cot, forward=tuple(f[0] for f in fwd))
        assert (again[0] == dv).all() and (again[2] == lams).all()


@pytest.mark.parametrize("dtype", [np.float32, np.longdouble])
def test_stepwise_adjoint_keeps_the_float_type(dtype):
    out = lc.adjoint_pass("depth-one", dtype, [0, 2])
    assert all(out[o].dtype == dtype for o in lc.OUTPUTS + ("munu",))


@pytest.mark.parametrize("name", lc.DENSE_NAMES)
def test_stored_bounds_are_32_times_the_measured_oracle_error(name):
    """each stored bound within [16, 64] x the freshly measured e64 / e32; hard caps as conditions"""
    measured = lc.measure(name)
    for dt, cap in (("float64", lc.FP64_CAP), ("float32", lc.FP32_CAP)):
        stored = lc.bounds(name, dt)
        assert set(stored) == set(lc.OUTPUTS)
        for o in lc.OUTPUTS:
            e = measured[dt][o]
            print(f"{name} {dt} {o}: e = {e:.3e}, bound = {stored[o]:.3e}")
            assert 16.0 * e <= stored[o] <= 64.0 * e, (name, dt, o, e, stored[o])
            assert stored[o] <= cap, (name, dt, o, stored[o])


@pytest.mark.parametrize("name", lc.SPARSE_NAMES)
def test_sparse_cases_inherit_a_bound_their_own_rounding_error_fits(name):
    """no longdouble run at these sizes: the bounds are the largest of the dense cases of the same depth (lc.bounds), and at least 16 x the
    difference of the fp64 and fp32 oracles on the case itself (that difference is e32 up to e64 << e32), scaled by u64 / u32 for
    the fp64 bound"""
    diff = lc.errors_between(lc.reference(name, "float32"), lc.reference(name, "float64"))
    ratio = rc.unit_roundoff("float64") / rc.unit_roundoff("float32")
    b32, b64 = lc.bounds(name, "float32"), lc.bounds(name, "float64")
    for o in lc.OUTPUTS:
        print(f"{name} {o}: fp64-fp32 oracle difference {diff[o]:.3e}, bounds {b32[o]:.3e} / {b64[o]:.3e}")
        assert b32[o] >= 16.0 * diff[o], (name, o, diff[o], b32[o])
        assert b64[o] >= 16.0 * diff[o] * ratio, (name, o, diff[o] * ratio, b64[o])
        assert b32[o] <= lc.FP32_CAP and b64[o] <= lc.FP64_CAP
