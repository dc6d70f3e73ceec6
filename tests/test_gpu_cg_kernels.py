"""csrc/mfx_cg.hip against the CPU oracle in longdouble, element by element, at every launch geometry of tests/_cg_cases.py:
mfx_pcg_solve (fixed-step and adaptive), mfx_pcg_solve_reortho, mfx_precond_apply and mfx_partial_cholesky -- one wave and four,
scalar and 16-byte accesses, one slice, two, three, 66 and 514, leading dimensions above n, preconditioner ranks 1 .. 1024 on
both sides of the re-orthogonalising depth, a frozen column inside a preconditioned batch, 257 blocks of pivot candidates,
exact ties and success = 0.

The C entry points are called directly, so that leading dimensions and raw workspaces are under the test's control.  The
bounds are cc.bounds: 32 x the oracle's own rounding error in the kernel's type, measured on the CPU
(tests/test_cg_cases_host.py), relative to the largest magnitude of the output per vector.  Outputs and workspaces live between
poisoned guard bands (tests/_guarded_ws.py): a store past n in a ragged last slice, or past the packed rows, lands in a band.

Every comparison prints `ratio <key> <type> <output> <error / bound>`; with MFX_CG_RATIO_LOG set to a file name the same lines
are appended there (profiles/cg_kernels_error_vs_bound.log is such a run)."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _cg_cases as cc
from _guarded_ws import GuardedWs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib
    from matfree_extensions.operators import CsrOp, DenseOp, RbfGramOp

DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
NAME = {torch.float64: "float64", torch.float32: "float32"}
NP = {torch.float64: np.float64, torch.float32: np.float32}
OK, INVALID, UNSUPPORTED = 0, -1, -2
SENTINEL = -7.0


def _dev(x, dtype):
    # row-major on the device whatever the layout of x: torch keeps the strides of a transposed numpy array, the kernels take raw pointers
    return torch.tensor(np.ascontiguousarray(x, dtype=np.float64), dtype=dtype, device=DEV).contiguous()


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _guarded(guards, shape, dtype, fill=None):
    """`shape` elements between bands of 0xFF bytes (NaN as floats); the tensor itself starts as NaN, or as `fill`"""
    guard = GuardedWs(0xFF)
    guards.append(guard)
    t = guard.take(int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(), DEV).view(dtype).view(*shape)
    if fill is not None:
        t.fill_(fill)
    return t


def _padded(rows, ld, dtype, pad=float("nan")):
    """(p, ld) on the device: `rows` (p, n) in the first n columns, `pad` in the others"""
    rows = np.asarray(rows)
    out = torch.full((rows.shape[0], ld), pad, dtype=dtype, device=DEV)
    out[:, : rows.shape[1]] = _dev(rows, dtype)
    return out


def _verify(guards):
    torch.cuda.synchronize()
    for guard in guards:
        guard.verify()


def _check(failures, key, dtype, output, got, ref, per_probe=True):
    """collects (output, error, bound) where max|got_b - ref_b| > bound * max|ref_b| for a vector b; prints every figure first"""
    bound = cc.bounds(key, NAME[dtype])[output]
    err = cc.rel_err(got, ref, per_probe)
    line = f"ratio {key} {NAME[dtype]} {output} {err / bound:.3f}  (error {err:.3e}, bound {bound:.3e})"
    print("    " + line)
    if os.environ.get("MFX_CG_RATIO_LOG"):
        with open(os.environ["MFX_CG_RATIO_LOG"], "a") as f:
            f.write(line + "\n")
    if not err <= bound:  # (also a NaN)
        failures.append((output, err, bound))


def _operator(s, dtype):
    """the descriptor of a case's operator (it keeps its device tensors alive)"""
    if s.kind == "dense":
        return DenseOp().descriptor((_dev(s.A, dtype),), dtype, s.n)
    op, vals, _ = CsrOp.from_coo(s.row, s.col, s.vals, s.n, DEV)
    return _owned(op, op.descriptor((vals.to(dtype),), dtype, s.n))


def _owned(op, desc):
    """A descriptor borrows the device pointers of tensors its operator object owns (the CSR structure, the Gram inputs X): the
    descriptor keeps the operator alive, or the allocator hands that memory to the next tensor while the kernels still read it."""
    desc._owner = op
    return desc


class _Pre:
    """Lt, minv and the shift on the device; `none` passes NULL pointers"""

    def __init__(self, s, dtype, none=False):
        self.rank = 0 if none else int(s.rank)
        self.lt = None if none else _dev(s.Lt, dtype)
        self.minv = None if none else _dev(s.minv, dtype)
        self.shift = None if none else _dev([cc.SHIFT], dtype)

    def args(self):
        return _lib.ptr(self.lt), self.rank, _lib.ptr(self.minv), _lib.ptr(self.shift)


def _pcg(desc, B, ldb, n, p, pre, maxiter, dtype, adaptive=0, atol=1.0, rtol=0.0):
    """one mfx_pcg_solve: (x, r, num_steps) with x and r packed (p, n) between guard bands, workspace of the exact size"""
    guards = []
    x, r = _guarded(guards, (p, n), dtype), _guarded(guards, (p, n), dtype)
    steps = torch.full((p,), -1, dtype=torch.int64, device=DEV)
    lib = _lib.get()
    ws = _guarded(guards, (int(lib.mfx_pcg_workspace_bytes(C.byref(desc), n, p, pre.rank)),), torch.uint8)
    before = _bits(B).clone()
    _lib.check(lib.mfx_pcg_solve(C.byref(desc), _lib.ptr(B), ldb, n, p, *pre.args(), maxiter, 0, atol, rtol, adaptive,
                                 _lib.ptr(x), _lib.ptr(r), _lib.ptr(steps), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
    _verify(guards)
    assert torch.equal(_bits(B), before)  # the right-hand sides and their padding are inputs
    return x, r, steps


# ------------------------------------------------------------------------------------------------
# fixed-step PCG
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("variant", ["plain", "pre"])
@pytest.mark.parametrize("name", cc.SOLVE_NAMES, ids=cc.solve_id)
def test_fixed_step_pcg_against_the_oracle(name, variant, dtype):
    """x and r of every right-hand side after exactly `steps` iterations.  The preconditioned runs take b with ldb = n + 3 and
    NaN in the padding: a read of it poisons the result, and x and r come back packed (their guard bands are intact)."""
    s = cc.solve_inputs(name)
    key = f"solve/{name}/{variant}"
    ref = cc.run(key)
    ldb = s.n + 3 if variant == "pre" else s.n
    x, r, steps = _pcg(_operator(s, dtype), _padded(s.B, ldb, dtype), ldb, s.n, s.p, _Pre(s, dtype, none=variant == "plain"), s.steps, dtype)
    assert steps.tolist() == [s.steps] * s.p
    failures = []
    _check(failures, key, dtype, "x", _host(x), ref["x"])
    _check(failures, key, dtype, "r", _host(r), ref["r"])
    assert not failures, failures


# ------------------------------------------------------------------------------------------------
# adaptive PCG
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_adaptive_pcg_stops_where_the_oracle_stops_and_freezes_columns(dtype):
    """Three columns that stop after 4, 1 and 2 steps, rank-5 preconditioner, two slices.  No stopping measure of the longdouble
    oracle is within [1/2, 2] (host test), so the step counts are the oracle's exactly.  A column solved alone gives the bits
    it has in the batch: k_pre_small, k_pre_finish, k_cg_xr and k_cg_dir leave a frozen column alone."""
    s = cc.adaptive_inputs()
    ref = cc.run("adaptive")
    desc, pre = _operator(s, dtype), _Pre(s, dtype)
    kw = dict(adaptive=1, atol=cc.ADAPTIVE_ATOL, rtol=cc.ADAPTIVE_RTOL)
    x, r, steps = _pcg(desc, _dev(s.B, dtype), s.n, s.n, s.p, pre, cc.ADAPTIVE_MAXITER, dtype, **kw)
    assert steps.tolist() == ref["num_steps"].tolist()
    failures = []
    _check(failures, "adaptive", dtype, "x", _host(x), ref["x"])
    assert not failures, failures
    for b in range(s.p):
        xb, rb, sb = _pcg(desc, _dev(s.B[b : b + 1], dtype), s.n, s.n, 1, pre, cc.ADAPTIVE_MAXITER, dtype, **kw)
        assert sb.item() == steps[b].item()
        assert torch.equal(_bits(xb[0]), _bits(x[b])) and torch.equal(_bits(rb[0]), _bits(r[b])), b


# ------------------------------------------------------------------------------------------------
# re-orthogonalising PCG
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("name", cc.REORTHO_NAMES)
def test_reortho_pcg_against_the_oracle(name, dtype):
    """x, r and the rows q_i = r_i / sqrt(r_i . z_i); workspace sized with rank = max(rank, num_matvecs) as include/mfx.h says.
    The rows are orthonormal in the M^-1 inner product (M^-1 applied in longdouble) to the bound of q."""
    s = cc.reortho_inputs(name)
    key = f"reortho/{name}"
    ref = cc.run(key)
    desc, pre = _operator(s, dtype), _Pre(s, dtype, none=s.rank == 0)
    guards = []
    x, r, q = _guarded(guards, (s.p, s.n), dtype), _guarded(guards, (s.p, s.n), dtype), _guarded(guards, (s.p, s.m, s.n), dtype)
    lib = _lib.get()
    ws = _guarded(guards, (int(lib.mfx_pcg_workspace_bytes(C.byref(desc), s.n, s.p, max(s.rank, s.m))),), torch.uint8)
    ldb = s.n + 3
    _lib.check(lib.mfx_pcg_solve_reortho(C.byref(desc), _lib.ptr(_padded(s.B, ldb, dtype)), ldb, s.n, s.p, *pre.args(), s.m, _lib.ptr(x),
                                         _lib.ptr(r), _lib.ptr(q), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
    _verify(guards)
    failures = []
    for out, t in (("x", x), ("r", r), ("q", q)):
        _check(failures, key, dtype, out, _host(t), ref[out])
    assert not failures, failures
    P = cc.preconditioner(s, np.longdouble) if s.rank else (lambda v: v)
    bound = cc.bounds(key, NAME[dtype])["q"]
    for b in range(s.p):
        Q = _host(q[b]).astype(np.longdouble)
        gram = Q @ np.stack([P(row) for row in Q]).T
        err = float(np.abs(gram - np.eye(s.m)).max())
        print(f"    column {b}: |Q M^-1 Q^T - I| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (b, err, bound)


# ------------------------------------------------------------------------------------------------
# mfx_precond_apply
# ------------------------------------------------------------------------------------------------
def _apply(s, pre, V, ldv, ldz, dtype):
    """z (p, ldz) of one mfx_precond_apply on the rows of V (p, ldv); z starts as SENTINEL everywhere"""
    p, lib = V.shape[0], _lib.get()
    guards = []
    z = _guarded(guards, (p, ldz), dtype, fill=SENTINEL)
    fake = _lib.Operator()
    fake.kind, fake.dtype, fake.n = _lib.OP_DENSE, _lib.dtype_code(dtype), s.n
    ws = _guarded(guards, (int(lib.mfx_pcg_workspace_bytes(C.byref(fake), s.n, p, s.rank)),), torch.uint8)
    before = _bits(V).clone()
    _lib.check(lib.mfx_precond_apply(fake.dtype, s.n, s.rank, _lib.ptr(pre.lt), _lib.ptr(pre.minv), _lib.ptr(pre.shift), _lib.ptr(V), ldv,
                                     _lib.ptr(z), ldz, p, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
    _verify(guards)
    assert torch.equal(_bits(V), before)
    assert (z[:, s.n :] == SENTINEL).all()  # the padding of z is not written
    return z[:, : s.n]


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("pads", [(3, 5), (4, 8)], ids=["ldv+3.ldz+5", "ldv+4.ldz+8"])
@pytest.mark.parametrize("name", cc.APPLY_NAMES, ids=cc.solve_id)
def test_precond_apply_with_padded_vectors(name, pads, dtype):
    """17 vectors with ldv = n + 3, ldz = n + 5 (strides that break the 16-byte alignment of every vector but the first), and
    n + 4, n + 8 (strides that keep it): NaN in the padding of v, a sentinel in that of z.  The same vector alone (p = 1:
    another workgroup size, another order of summation) agrees with its row of the batch within twice the bound."""
    s = cc.solve_inputs(name)
    key = f"apply/{name}"
    ref, pre = cc.run(key)["z"], _Pre(s, dtype)
    ldv, ldz = s.n + pads[0], s.n + pads[1]
    z = _apply(s, pre, _padded(s.V, ldv, dtype), ldv, ldz, dtype)
    failures = []
    _check(failures, key, dtype, "z", _host(z), ref)
    b = 5
    z1 = _apply(s, pre, _padded(s.V[b : b + 1], ldv, dtype), ldv, ldz, dtype)
    _check(failures, key, dtype, "z", _host(z1), ref[b : b + 1])
    assert not failures, failures
    bound = cc.bounds(key, NAME[dtype])["z"]
    assert cc.rel_err(_host(z1), _host(z[b : b + 1])) <= 2.0 * bound


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_lowrank_apply_with_minv_and_one_over_s_is_precond_apply(dtype):
    s = cc.solve_inputs("wg256-vector")
    pre, lib = _Pre(s, dtype), _lib.get()
    V = _dev(s.V, dtype)
    z = _apply(s, pre, V, s.n, s.n, dtype)
    z2 = torch.full_like(V, float("nan"))
    code = _lib.dtype_code(dtype)
    ws = torch.empty(int(lib.mfx_lowrank_workspace_bytes(code, s.n, s.rank, cc.APPLY_P)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.mfx_lowrank_apply(code, s.n, s.rank, _lib.ptr(pre.lt), _lib.ptr(pre.minv), _lib.ptr(_dev([1.0 / cc.SHIFT], dtype)),
                                     _lib.ptr(V), s.n, _lib.ptr(z2), s.n, cc.APPLY_P, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert cc.rel_err(_host(z2), _host(z)) <= 2.0 * cc.bounds("apply/wg256-vector", NAME[dtype])["z"]


# ------------------------------------------------------------------------------------------------
# mfx_partial_cholesky
# ------------------------------------------------------------------------------------------------
def _cholesky(desc, n, rank, pivot, with_noise, dtype):
    guards, lib = [], _lib.get()
    lt = _guarded(guards, (rank, n), dtype)
    pivots = torch.full((rank,), -1, dtype=torch.int64, device=DEV)
    success = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = _guarded(guards, (int(lib.mfx_pcg_workspace_bytes(C.byref(desc), n, 1, rank)),), torch.uint8)
    _lib.check(lib.mfx_partial_cholesky(C.byref(desc), rank, pivot, with_noise, _lib.ptr(lt), _lib.ptr(pivots), _lib.ptr(success),
                                        _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
    _verify(guards)
    return lt, pivots.tolist(), int(success.item())


def _dense_desc(A, dtype):
    return DenseOp().descriptor((_dev(A, dtype),), dtype, len(A))


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("name", cc.CHOL_NAMES)
def test_partial_cholesky_against_the_oracle(name, dtype):
    """Pivots equal the longdouble oracle's exactly (every step is won by a relative 1e-3, or is the exact tie of a Gram
    diagonal: host test), Lt within its bound row by row, success = 1."""
    s = cc.chol_inputs(name)
    key = f"chol/{name}"
    ref = cc.run(key)
    if s.kind == "dense":
        desc = _dense_desc(s.A, dtype)
    else:
        params = (_dev([cc.GRAM_LS], dtype), _dev([cc.GRAM_OS], dtype), _dev([cc.GRAM_NOISE], dtype))
        op = RbfGramOp(_dev(s.X, dtype), precision="fp32")
        desc = _owned(op, op.descriptor(params, dtype, s.n))
    lt, pivots, success = _cholesky(desc, s.n, s.rank, s.pivot, s.with_noise, dtype)
    assert pivots == ref["pivots"].tolist() and success == 1 == int(ref["success"])
    failures = []
    _check(failures, key, dtype, "Lt", _host(lt), ref["Lt"])
    assert not failures, failures


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_partial_cholesky_breaks_exact_ties_like_the_oracle(dtype):
    """small integers, every operation exact: ties between rows of different 256-row blocks go to the first index, and the
    factor equals the oracle's bit for bit"""
    A = cc.tie_matrix()
    rank = len(cc.TIE_PIVOTS)
    col, diag = cc.dense_columns(A)
    L, ref_pivots, ref_success, _ = cc.cholesky_partial(col, diag, len(A), rank, np.float64, True)
    lt, pivots, success = _cholesky(_dense_desc(A, dtype), len(A), rank, 1, 0, dtype)
    assert pivots == ref_pivots.tolist() == list(cc.TIE_PIVOTS) and success == int(ref_success) == 1
    assert (_host(lt) == L.T).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_partial_cholesky_reports_a_rank_deficient_matrix(dtype):
    """v v^T of small integers: success = 0 like the oracle's, the column before the failing step is exact"""
    A, v = cc.deficient_matrix()
    col, diag = cc.dense_columns(A)
    for pivot, rank in ((0, 3), (1, 2)):
        L, ref_pivots, ref_success, _ = cc.cholesky_partial(col, diag, len(A), rank, np.float64, bool(pivot))
        lt, pivots, success = _cholesky(_dense_desc(A, dtype), len(A), rank, pivot, 0, dtype)
        assert success == int(ref_success) == 0
        assert pivots[0] == ref_pivots[0] and (pivot or pivots == ref_pivots.tolist())
        assert (_host(lt[0]) == L[:, 0]).all() and (L[:, 0] == v).all()


# ------------------------------------------------------------------------------------------------
# refusals: return codes only, before any launch
# ------------------------------------------------------------------------------------------------
def test_refusals_by_return_code():
    dtype = torch.float32
    s = cc.solve_inputs("wg256-vector")
    n, p, lib = s.n, 2, _lib.get()
    desc, pre = _operator(s, dtype), _Pre(s, dtype)
    B, x, r = _dev(s.B[:p], dtype), torch.full((p, n), SENTINEL, dtype=dtype, device=DEV), torch.full((p, n), SENTINEL, dtype=dtype, device=DEV)
    q = torch.full((p, 8, n), SENTINEL, dtype=dtype, device=DEV)
    ws = torch.empty(int(lib.mfx_pcg_workspace_bytes(C.byref(desc), n, p, 1024)), dtype=torch.uint8, device=DEV)
    big = torch.zeros((1025, n), dtype=dtype, device=DEV)  # rank 1025 <= n = 1028: the limit itself, not rank > n, refuses
    stream = _lib.stream_ptr(DEV)

    def solve(ldb=n, lt=pre.lt, rank=pre.rank):
        return lib.mfx_pcg_solve(C.byref(desc), _lib.ptr(B), ldb, n, p, _lib.ptr(lt), rank, _lib.ptr(pre.minv), _lib.ptr(pre.shift), 2, 0,
                                 1.0, 0.0, 0, _lib.ptr(x), _lib.ptr(r), None, _lib.ptr(ws), ws.numel(), stream)

    def reortho(m, ldb=n, rank=pre.rank, lt=pre.lt):
        return lib.mfx_pcg_solve_reortho(C.byref(desc), _lib.ptr(B), ldb, n, p, _lib.ptr(lt), rank, _lib.ptr(pre.minv),
                                         _lib.ptr(pre.shift), m, _lib.ptr(x), _lib.ptr(r), _lib.ptr(q), _lib.ptr(ws), ws.numel(), stream)

    def apply(ldv=n, ldz=n, rank=pre.rank, lt=pre.lt):
        return lib.mfx_precond_apply(_lib.MFX_F32, n, rank, _lib.ptr(lt), _lib.ptr(pre.minv), _lib.ptr(pre.shift), _lib.ptr(B), ldv,
                                     _lib.ptr(x), ldz, p, _lib.ptr(ws), ws.numel(), stream)

    assert solve(rank=1025, lt=big) == UNSUPPORTED and reortho(8, rank=1025, lt=big) == UNSUPPORTED and apply(rank=1025, lt=big) == UNSUPPORTED
    assert solve(rank=n + 1, lt=big) == INVALID and apply(rank=n + 1, lt=big) == INVALID and apply(rank=0) == INVALID
    assert solve(ldb=n - 1) == INVALID and reortho(8, ldb=n - 1) == INVALID
    assert apply(ldv=n - 1) == INVALID and apply(ldz=n - 1) == INVALID
    assert reortho(0) == INVALID and reortho(1025) == INVALID
    torch.cuda.synchronize()
    assert (x == SENTINEL).all() and (r == SENTINEL).all() and (q == SENTINEL).all()  # nothing was launched
    assert solve() == OK and apply() == OK and reortho(8) == OK
    torch.cuda.synchronize()
