"""The dense and CSR operator kernels (k_dense_apply, k_dense_apply_t, k_dense_grad, k_csr_apply, k_csr_grad) through
mfx_op_apply / mfx_op_vjp_params with the descriptor filled directly -- leading dimensions, row blocks, accumulation into a
non-zero buffer, ragged rows -- and the fused CSR step head k_csr_step at every launch geometry through the Krylov drivers.

References are fp64 numpy on the dense matrix (tests/_ragged_csr.py); the bounds are apply_bound and grad_bound of that file,
componentwise.  Every output lives inside a padded buffer filled with a sentinel: what the kernel does not own must come back
bitwise unchanged."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _ragged_csr as rc
from oracle import slq_oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib, arnoldi, lanczos
    from matfree_extensions.operators import CsrOp, DenseOp

DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
NAME = {torch.float64: "float64", torch.float32: "float32"}
PAD = 16  # sentinel elements before and after every output
SENTINEL = -12345.6789


def _dev(x, dtype):
    return torch.tensor(np.asarray(x), dtype=dtype, device=DEV)


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _rounded(x, dtype):
    """fp64 numpy values that are exactly representable in dtype: the reference is formed on what the kernel reads"""
    return np.asarray(x, dtype=np.float32).astype(np.float64) if dtype == torch.float32 else np.asarray(x, dtype=np.float64)


def _strided(x, ld, dtype):
    """device copy of x (rows, cols) with leading dimension ld >= cols (the gaps hold the sentinel)"""
    rows, cols = x.shape
    buf = torch.full((rows, ld), SENTINEL, dtype=dtype, device=DEV)
    buf[:, :cols] = _dev(x, dtype)
    return buf


class _Guarded:
    """a (rows, cols) output of leading dimension ld inside a sentinel-filled buffer; `fill` pre-loads the owned region"""

    def __init__(self, rows, cols, ld, dtype, fill=None):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.buf = torch.full((PAD + rows * ld + PAD,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[PAD : PAD + rows * ld].view(rows, ld)
        if fill is not None:
            self.view[:, :cols] = _dev(fill, dtype)
        self.before = self.buf.clone()

    def ptr(self):
        return self.view.data_ptr()

    def assert_untouched_outside(self, written):
        """written: bool (rows, cols) mask of the entries the kernel owns; everything else is bitwise what it was"""
        mask = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        mask[PAD : PAD + self.rows * self.ld].view(self.rows, self.ld)[:, : self.cols] = torch.as_tensor(written, device=DEV)
        bits = torch.int64 if self.buf.dtype == torch.float64 else torch.int32
        assert torch.equal(self.buf.view(bits)[~mask], self.before.view(bits)[~mask]), "the kernel wrote outside its output"

    def values(self):
        return _host(self.view[:, : self.cols])


def _apply(desc, x, ldx, y, ldy, p, transpose, n):
    ws = _lib.workspace(desc, n, 1, p, DEV)
    _lib.check(_lib.get().mfx_op_apply(C.byref(desc), x.data_ptr(), ldx, y.ptr(), ldy, p, transpose, _lib.ptr(ws), ws.numel(),
                                       _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()


def _vjp(desc, L, ldl, R, ldr, batch, gs, n):
    ws = _lib.workspace(desc, n, 1, batch, DEV)
    _lib.check(_lib.get().mfx_op_vjp_params(C.byref(desc), L.data_ptr(), ldl, R.data_ptr(), ldr, batch, C.byref(gs), _lib.ptr(ws),
                                            ws.numel(), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()


def _assert_within(got, ref, bound, what):
    err = np.abs(got - ref)
    bad = err > bound
    assert not bad.any(), (what, "worst error / bound", float((err[bad] / np.maximum(bound[bad], 1e-300)).max()), "at", np.argwhere(bad)[:4].tolist())


def _blocks(n, candidates):
    """(row0, nrows) of the candidates that fit an n-row operator, without repeats"""
    out = []
    for row0, nrows in candidates:
        if row0 >= 0 and nrows >= 1 and row0 + nrows <= n and (row0, nrows) not in out:
            out.append((row0, nrows))
    return out


def _dense_blocks(n):
    return _blocks(n, [(0, n), (1, 1), (n - 1, 1), (3, 64), (61, 70)])


def _csr_blocks(n):
    return _blocks(n, [(0, n), (0, 1), (n - 1, 1), (5, 32), (17, 40)])


# ------------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------------
DENSE_N = [1, 3, 63, 64, 65, 130, 257]


@functools.lru_cache(maxsize=None)
def _dense_inputs(n, dtype):
    rng = np.random.default_rng(31 * n + 1)
    W = _rounded(rng.standard_normal((n, n + 3)), dtype)  # A is the view W[:, :n]
    X = _rounded(rng.standard_normal((9, n)), dtype)
    return W, X


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("wide", [False, True], ids=["lda=n", "lda=n+3"])
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("n", DENSE_N)
def test_dense_apply_with_leading_dimensions_and_row_blocks(n, transpose, wide, dtype):
    """k_dense_apply (one wave per row, 4 rows per workgroup) and k_dense_apply_t (64 columns per workgroup), 4 probes per pass:
    p in {1, 4, 5, 9}, lda in {n, n + 3}, ldx = n + 5, ldy = nrows + 2, row blocks across the 4-row and 64-column edges"""
    W, X = _dense_inputs(n, dtype)
    A = W[:, :n]
    Wd = _dev(W, dtype)
    Ad = Wd[:, :n] if wide else torch.empty((n, n), dtype=dtype, device=DEV).copy_(Wd[:, :n])
    assert Ad.stride(0) == (n + 3 if wide else n)
    u = rc.unit_roundoff(NAME[dtype])
    ref_all, mag_all = rc.apply_ref(A, X, bool(transpose))
    op = DenseOp()
    for p in (1, 4, 5, 9):
        xd = _strided(X[:p], n + 5, dtype)
        for row0, nrows in _dense_blocks(n):
            desc = op.descriptor((Ad,), dtype, n)
            desc.row0, desc.nrows = row0, nrows
            y = _Guarded(p, nrows, nrows + 2, dtype)
            _apply(desc, xd, n + 5, y, nrows + 2, p, transpose, n)
            y.assert_untouched_outside(np.ones((p, nrows), dtype=bool))
            sl = slice(row0, row0 + nrows)
            _assert_within(y.values(), ref_all[:p, sl], rc.apply_bound(n, u, mag_all[:p, sl]), (p, row0, nrows))


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("batch", [1, 7])
@pytest.mark.parametrize("n", DENSE_N)
def test_dense_grad_accumulates_into_its_row_block_only(n, batch, dtype):
    """k_dense_grad (16 x 16 tiles): dA[row0 + i][j] += sum_b L[b][i] R[b][j] on a pre-filled dA; rows outside the block and the
    padding around dA bitwise unchanged"""
    rng = np.random.default_rng(57 * n + batch)
    R = _rounded(rng.standard_normal((batch, n)), dtype)
    Lfull = _rounded(rng.standard_normal((batch, n)), dtype)
    prefill = _rounded(rng.standard_normal((n, n)), dtype)
    u = rc.unit_roundoff(NAME[dtype])
    op = DenseOp()
    Ad = torch.zeros((n, n), dtype=dtype, device=DEV)  # the matrix itself is not read by the sweep
    rd = _strided(R, n + 5, dtype)
    for row0, nrows in _dense_blocks(n):
        L = Lfull[:, :nrows]
        ld = _strided(L, nrows + 1, dtype)
        desc = op.descriptor((Ad,), dtype, n)
        desc.row0, desc.nrows = row0, nrows
        dA = _Guarded(n, n, n, dtype, fill=prefill)
        gs = _lib.OpGrads()
        gs.dense_a = dA.ptr()
        _vjp(desc, ld, nrows + 1, rd, n + 5, batch, gs, n)
        owned = np.zeros((n, n), dtype=bool)
        owned[row0 : row0 + nrows] = True
        dA.assert_untouched_outside(owned)
        ref, mag = rc.outer_ref(L, R)
        sl = slice(row0, row0 + nrows)
        _assert_within(dA.values()[sl], prefill[sl] + ref, rc.grad_bound(batch, u, mag, prefill[sl]), (row0, nrows))


# ------------------------------------------------------------------------------------------------
# CSR on ragged matrices
# ------------------------------------------------------------------------------------------------
CSR_N = [1, 31, 32, 33, 1000]


@functools.lru_cache(maxsize=None)
def _csr_inputs(n, dtype):
    rng = np.random.default_rng(91 * n + 7)
    row, col, vals = rc.ragged_csr(n, rng, **({"lengths": (1,)} if n == 1 else {}))  # (n = 1: the one entry, not the empty pattern)
    vals = _rounded(vals, dtype)
    X = _rounded(rng.standard_normal((7, n)), dtype)
    Y = _rounded(rng.standard_normal((7, n)), dtype)
    return row, col, vals, rc.dense_of(row, col, vals, n), X, Y


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("n", CSR_N)
def test_csr_apply_on_ragged_rows_with_row_blocks(n, transpose, dtype):
    """k_csr_apply (8 lanes per row, 32 rows per workgroup): rows of 0 .. 64 entries -- empty rows, whole rounds of 8, ragged
    tails -- forward and through the transposed structure with t_perm, p in {1, 3}, row blocks, padded ldx / ldy"""
    row, col, vals, A, X, _ = _csr_inputs(n, dtype)
    op, vd, order = CsrOp.from_coo(row, col, vals, n, DEV)
    vd = vd.to(dtype)
    rows, cols = rc.row_and_col_lengths(row, col, n)
    terms = cols if transpose else rows
    u = rc.unit_roundoff(NAME[dtype])
    ref_all, mag_all = rc.apply_ref(A, X, bool(transpose))
    for p in (1, 3):
        xd = _strided(X[:p], n + 5, dtype)
        for row0, nrows in _csr_blocks(n):
            desc = op.descriptor((vd,), dtype, n)
            desc.row0, desc.nrows = row0, nrows
            y = _Guarded(p, nrows, nrows + 2, dtype)
            _apply(desc, xd, n + 5, y, nrows + 2, p, transpose, n)
            y.assert_untouched_outside(np.ones((p, nrows), dtype=bool))
            sl = slice(row0, row0 + nrows)
            got = y.values()
            assert (got[:, terms[sl] == 0] == 0.0).all(), "an empty row must give exactly 0"
            _assert_within(got, ref_all[:p, sl], rc.apply_bound(terms[sl][None, :], u, mag_all[:p, sl]), (p, row0, nrows))


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("batch", [1, 7])
@pytest.mark.parametrize("n", CSR_N)
def test_csr_grad_accumulates_into_the_entries_of_its_row_block_only(n, batch, dtype):
    """k_csr_grad (one thread per stored entry): dval[e] += sum_b L[b][row_e - row0] R[b][col_e] for the entries of the block's rows,
    on a pre-filled dval, in the stored order CsrOp.from_coo returns"""
    row, col, vals, _, X, Y = _csr_inputs(n, dtype)
    op, vd, order = CsrOp.from_coo(row, col, vals, n, DEV)
    vd, order = vd.to(dtype), order.numpy()
    srow, scol = row[order], col[order]
    nnz = len(row)
    R, Lfull = X[:batch], Y[:batch]
    prefill = _rounded(np.random.default_rng(n + batch).standard_normal(nnz), dtype)
    u = rc.unit_roundoff(NAME[dtype])
    rd = _strided(R, n + 5, dtype)
    for row0, nrows in _csr_blocks(n):
        L = Lfull[:, :nrows]
        ld = _strided(L, nrows + 1, dtype)
        desc = op.descriptor((vd,), dtype, n)
        desc.row0, desc.nrows = row0, nrows
        dval = _Guarded(1, nnz, nnz, dtype, fill=prefill[None, :])
        gs = _lib.OpGrads()
        gs.val = dval.ptr()
        _vjp(desc, ld, nrows + 1, rd, n + 5, batch, gs, n)
        owned = (srow >= row0) & (srow < row0 + nrows)
        dval.assert_untouched_outside(owned[None, :])
        ref, mag = rc.outer_ref(L, R)
        e = np.flatnonzero(owned)
        ref_e, mag_e = ref[srow[e] - row0, scol[e]], mag[srow[e] - row0, scol[e]]
        _assert_within(dval.values()[0, e], prefill[e] + ref_e, rc.grad_bound(batch, u, mag_e, prefill[e]), (row0, nrows))


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_csr_operator_without_stored_values_is_the_zero_matrix(dtype):
    """n = 5, nnz = 0: mfx_op_apply gives y == 0 both ways and mfx_op_vjp_params returns MFX_OK without launching the zero-sized
    grid of k_csr_grad"""
    n, p = 5, 3
    op = CsrOp(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n, device=DEV)
    assert op.nnz == 0 and op.max_row_nnz == 0
    vd = torch.zeros(0, dtype=dtype, device=DEV)
    X = np.random.default_rng(5).standard_normal((p, n))
    xd = _strided(X, n + 5, dtype)
    for transpose in (0, 1):
        y = _Guarded(p, n, n + 2, dtype)
        _apply(op.descriptor((vd,), dtype, n), xd, n + 5, y, n + 2, p, transpose, n)
        y.assert_untouched_outside(np.ones((p, n), dtype=bool))
        assert (y.values() == 0.0).all()
    # the sweep: through the operator's own gradient struct (no values: a null pointer) and with a live one-element buffer
    gs, _ = op.new_grads(vd)
    _vjp(op.descriptor((vd,), dtype, n), xd, n + 5, xd, n + 5, p, gs, n)
    g = _Guarded(1, 1, 1, dtype)
    gs = _lib.OpGrads()
    gs.val = g.ptr()
    _vjp(op.descriptor((vd,), dtype, n), xd, n + 5, xd, n + 5, p, gs, n)
    g.assert_untouched_outside(np.zeros((1, 1), dtype=bool))


# ------------------------------------------------------------------------------------------------
# the fused CSR step at every geometry, through the drivers
# ------------------------------------------------------------------------------------------------
def _close(a, b, rtol, atol_rel):
    a, b = _host(a), np.asarray(b)
    ok = np.allclose(a, b, rtol=rtol, atol=atol_rel * max(np.abs(b).max(), 1e-300))
    if not ok:
        print("max abs err", np.abs(a - b).max(), "scale", np.abs(b).max())
    return ok


def _hessenberg_against_the_oracle(row, col, vals, V, k, reortho, op, vt, order, probes, dtypes=DTYPES):
    """arnoldi.hessenberg forward + adjoint with cotangents on Q, H, r and c: fp64 against the oracle for `probes`, with the
    tolerances of test_hessenberg_shape_sweep_csr_against_the_oracle; fp32 against fp64 for all probes under the scale rule of
    test_hessenberg_shape_sweep_fp32_batched"""
    p, n = V.shape
    o = orc.CooOp(row, col, n)
    outs = {}
    for dtype in dtypes:
        v_ = vt.to(dtype).requires_grad_(True)
        x_ = _dev(V, dtype).requires_grad_(True)
        Q, H, rr, cc = arnoldi.hessenberg(op, k, reortho=reortho)(x_, v_)
        g = torch.Generator(device=DEV).manual_seed(5)
        cot = [torch.randn(t.shape, dtype=torch.float64, device=DEV, generator=g).to(dtype) for t in (Q, H, rr, cc)]
        dv, dvals = torch.autograd.grad((Q, H, rr, cc), (x_, v_), cot)
        outs[dtype] = [t.detach().double() for t in (Q, H, rr, cc, dv, dvals)]
        if dtype == torch.float64:
            cot64 = [_host(t) for t in cot]
    Q, H, rr, cc, dv, dvals = outs[torch.float64]
    dvals_ref = 0.0
    for b in probes:
        Qo, Ho, ro, co = orc.arnoldi_forward(o, k, V[b], vals, reortho=reortho)
        assert _close(Q[b], Qo, 1e-9, 1e-9) and _close(H[b], Ho, 1e-9, 1e-9) and _close(cc[b], co, 1e-10, 1e-10), b
        assert np.allclose(_host(rr[b]), ro, rtol=1e-8, atol=1e-9 * max(np.abs(ro).max(), 1e-30) + 1e-13), b
        dv_ref, (dp,) = orc.arnoldi_adjoint(o, (vals,), Q=Qo, H=Ho, r=ro, c=co, reortho=reortho, dQ=cot64[0][b], dH=cot64[1][b],
                                            dr=cot64[2][b], dc=cot64[3][b])
        assert _close(dv[b], dv_ref, 1e-7, 1e-8), b
        dvals_ref = dvals_ref + dp
    if len(probes) == p:  # the gradient of the stored values sums over ALL probes
        assert _close(dvals, dvals_ref[order.numpy()], 1e-7, 1e-8)
    if torch.float32 in outs:
        for a32, a64 in zip(outs[torch.float32], outs[torch.float64]):
            scale = a64.abs().max().item()
            assert torch.allclose(a32, a64, rtol=2e-3, atol=2e-4 * scale), (a32 - a64).abs().max().item() / scale


def _tridiag_against_the_oracle(row, col, vals, V, k, op, vt, probes):
    """lanczos.tridiag(reortho="none") forward, fp64, with the tolerances of test_csr_skewed_rows_pick_the_step_kernel_by_the_longest_row"""
    n = V.shape[1]
    o = orc.CooOp(row, col, n)
    (xs, (al, be)), (xl, bl) = lanczos.tridiag(op, k, reortho="none")(_dev(V, torch.float64), vt.double())
    for b in probes:
        (xo, (ao, bo)), (xlo, blo) = orc.tridiag(o, k, V[b], vals, reortho="none")
        assert _close(al[b], ao, 1e-9, 1e-9) and _close(xs[b], xo, 1e-8, 1e-8) and _close(xl[b], xlo, 1e-8, 1e-8), b
        assert _close(torch.cat([be[b], bl[b : b + 1]]), np.concatenate([bo, [blo]]), 1e-9, 1e-9), b


def _case_id(case):
    name, n, p = case[:3]
    return f"{name}-n{n}-p{p}-f32:{rc.geometry_name(n, p, 'float32')}-f64:{rc.geometry_name(n, p, 'float64')}"


@pytest.mark.parametrize("reortho", ["full", "none"])
@pytest.mark.parametrize("k", rc.KRYLOV_DEPTHS)
@pytest.mark.parametrize("case", rc.KRYLOV_CASES, ids=_case_id)
def test_fused_csr_step_at_every_geometry(case, k, reortho):
    """k_csr_step on ragged matrices with an empty run of rows (a whole workgroup's slice wherever n has a second one), at the five
    (workgroup, VEC, EPT) geometries the case id names per dtype: forward, the transposed structure in the adjoint, and the
    three-term recurrence.  tests/test_ragged_csr_host.py asserts the geometries and the no-breakdown margins of these inputs."""
    name, n, p, _, _ = case
    row, col, vals, V = rc.krylov_case(name)
    op, vt, order = CsrOp.from_coo(row, col, vals, n, DEV)
    assert op.max_row_nnz == 64  # both structures on the fused step
    probes = rc.oracle_probes(p)
    _hessenberg_against_the_oracle(row, col, vals, V, k, reortho, op, vt, order, probes)
    if reortho == "none":
        _tridiag_against_the_oracle(row, col, vals, V, min(k, 8), op, vt, probes)


@pytest.mark.parametrize("reortho", ["full", "none"])
@pytest.mark.parametrize("longest,stated", [(64, 64), (65, 65), (200, 0)], ids=["64-fused", "65-eight-lanes", "200-unstated-mean-rule-fused"])
def test_fused_step_switch_at_64_and_65_and_by_the_mean_rule(longest, stated, reortho):
    """max_row_nnz == 64 keeps the fused step, 65 takes the 8-lanes-per-row kernels, and an operator that does not state its longest
    row (max_row_nnz = 0) is judged on the mean: fused, with one thread walking a row of 200 entries.  All against the oracle."""
    n, k = 1536, 9
    row, col, vals = rc.krylov_switch_case(longest)
    V = rc.krylov_switch_vector()[None, :]
    op, vt, order = CsrOp.from_coo(row, col, vals, n, DEV)
    assert op.max_row_nnz == longest
    if stated == 0:
        assert op.nnz <= 24 * n
        op.max_row_nnz = 0
    _hessenberg_against_the_oracle(row, col, vals, V, k, reortho, op, vt, order, [0])
    if reortho == "none":
        _tridiag_against_the_oracle(row, col, vals, V, 8, op, vt, [0])
