"""f(A) v on the Lanczos path: the four kernels one by one on host-generated inputs, the workspace contract of
``mfx_basis_combine_bwd``, ``lanczos.funm_spd`` / ``pde_util.expm_lanczos`` / ``gp_util.gram_funm`` end to end, their gradients against
autograd through the torch-CPU fp64 restatement (tests/_funm_restatement.py), and the refusals.

Tolerances are the parity bars of DESIGN.md section 0: fp64 against a CPU fp64 restatement 1e-10, fp32 against fp64 1e-4, fp64 gradients
1e-8 -- all relative to the largest component of the reference."""

import math

import pytest
import torch

import _funm_restatement as rs
from _guarded_ws import GuardedWs
from matfree_extensions import _lib, lanczos
from matfree_extensions.operators import CsrOp, DenseOp, RowShardedOp
from matfree_extensions.util import gp_util, pde_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
MFX_ERR_WORKSPACE = -4
VALUE_TOL = {F64: 1e-10, F32: 1e-4}
GRAD_TOL = 1e-8
MATFUNS = {
    "sqrt": torch.sqrt,
    "reciprocal": torch.reciprocal,
    "exp": lambda lam: torch.exp(-0.3 * lam),
    "log": torch.log,
}


def relerr(got, ref):
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite result"
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def rand(shape, seed, dtype=F64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64).to(dtype)


def inv_softplus(v):
    return math.log(math.expm1(v))


# ---------------------------------------------------------------------------------------------------------------------------
# raw entry points
# ---------------------------------------------------------------------------------------------------------------------------
def _stream():
    return _lib.stream_ptr(DEV)


def raw_coeffs(evals, evecs, fvals, scale):
    p, k = evals.shape
    out = torch.empty_like(evals)
    _lib.check(_lib.get().mfx_funm_coeffs(_lib.ptr(evals), _lib.ptr(evecs), _lib.ptr(fvals), _lib.ptr(scale), p, k, _lib.dtype_code(evals.dtype),
                                          _lib.ptr(out), _stream()))
    return out


def raw_coeffs_bwd(evals, evecs, fvals, dfvals, dc, scale):
    p, k = evals.shape
    ld = max(k - 1, 1) + 2  # a leading dimension beyond the width: the padding must survive
    dalpha = torch.empty_like(evals)
    dbeta = torch.full((p, ld), -77.0, dtype=evals.dtype, device=DEV)
    dscale = torch.empty((p,), dtype=evals.dtype, device=DEV)
    _lib.check(_lib.get().mfx_funm_coeffs_bwd(_lib.ptr(evals), _lib.ptr(evecs), _lib.ptr(fvals), _lib.ptr(dfvals), _lib.ptr(dc), _lib.ptr(scale),
                                              p, k, _lib.dtype_code(evals.dtype), _lib.ptr(dalpha), _lib.ptr(dbeta), ld, _lib.ptr(dscale), _stream()))
    assert bool((dbeta[:, k - 1:] == -77.0).all()), "dbeta written beyond its k - 1 entries"
    return dalpha, dbeta[:, : k - 1], dscale


def raw_combine(Q, c):
    p, k, n = Q.shape
    y = torch.empty((p, n), dtype=Q.dtype, device=DEV)
    _lib.check(_lib.get().mfx_basis_combine(_lib.ptr(Q), _lib.ptr(c), n, k, p, _lib.dtype_code(Q.dtype), _lib.ptr(y), _stream()))
    return y


def combine_ws_bytes(Q):
    p, k, n = Q.shape
    need = int(_lib.get().mfx_basis_combine_workspace_bytes(n, k, p, _lib.dtype_code(Q.dtype)))
    assert need > 0
    return need


def raw_combine_bwd(Q, c, dy, want_q=True, want_c=True, ws=None, ws_bytes=None, check=True):
    p, k, n = Q.shape
    dQ = torch.full((p, k, n), -77.0, dtype=Q.dtype, device=DEV) if want_q else None
    dc = torch.full((p, k), -77.0, dtype=Q.dtype, device=DEV) if want_c else None
    if ws is None:
        ws = torch.empty(combine_ws_bytes(Q), dtype=torch.uint8, device=DEV)
    rc = _lib.get().mfx_basis_combine_bwd(_lib.ptr(Q), _lib.ptr(c), _lib.ptr(dy), n, k, p, _lib.dtype_code(Q.dtype), _lib.ptr(dQ), _lib.ptr(dc),
                                          _lib.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
    if check:
        _lib.check(rc)
    return dQ, dc, rc


# ---------------------------------------------------------------------------------------------------------------------------
# mfx_funm_coeffs / _bwd
# ---------------------------------------------------------------------------------------------------------------------------
def _eigen_problem(p, k, dtype, seed):
    """random orthogonal evecs, separated evals in [0.5, 3] in random order, f = sqrt; everything rounded to `dtype` first"""
    g = torch.Generator().manual_seed(seed)
    U = torch.stack([torch.linalg.qr(torch.randn(k, k, generator=g, dtype=F64))[0] for _ in range(p)]).to(dtype)
    lam = torch.stack([torch.linspace(0.5, 3.0, k, dtype=F64)[torch.randperm(k, generator=g)] for _ in range(p)]).to(dtype)
    fl, dfl = torch.sqrt(lam.to(F64)).to(dtype), (0.5 / torch.sqrt(lam.to(F64))).to(dtype)
    dc = torch.randn(p, k, generator=g, dtype=F64).to(dtype)
    scale = (0.5 + torch.rand(p, generator=g, dtype=F64)).to(dtype)
    return lam, U, fl, dfl, dc, scale


def _coeffs_reference(lam, U, fl, dfl, dc, scale, rel_tol):
    lam, U, fl, dfl, dc, scale = (t.to(F64) for t in (lam, U, fl, dfl, dc, scale))
    c = torch.stack([scale[b] * (U[b] @ (fl[b] * U[b][0])) for b in range(lam.shape[0])])
    parts = [rs.coeffs_vjp(lam[b], U[b], fl[b], dfl[b], dc[b], scale[b], rel_tol) for b in range(lam.shape[0])]
    return c, torch.stack([q[0] for q in parts]), torch.stack([q[1] for q in parts]), torch.stack([q[2] for q in parts])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("k", [1, 2, 7, 120, 121, 130])
def test_coeffs_and_their_vjp_against_the_cpu(k, p, dtype):
    host = _eigen_problem(p, k, dtype, 100 * k + p)
    ref = _coeffs_reference(*host, rel_tol=1e-13 if dtype == F64 else 1e-6)
    lam, U, fl, dfl, dc, scale = (t.to(DEV).contiguous() for t in host)
    c = raw_coeffs(lam, U, fl, scale)
    dalpha, dbeta, dscale = raw_coeffs_bwd(lam, U, fl, dfl, dc, scale)
    torch.cuda.synchronize()
    tol = VALUE_TOL[dtype]
    for what, got, want in (("coeffs", c, ref[0]), ("dalpha", dalpha, ref[1]), ("dscale", dscale, ref[3])) + ((("dbeta", dbeta, ref[2]),) if k > 1 else ()):
        err = relerr(got, want)
        print(f"k={k} p={p} {dtype}: {what} {err:.2e}")
        assert err <= tol, (what, err)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_coeffs_vjp_on_a_fully_degenerate_spectrum(dtype):
    """evecs = I, every eigenvalue = a: dalpha = f'(a) dc_0 e_0, dbeta_0 = f'(a) dc_1, every other dbeta 0, nothing NaN / Inf"""
    k, a = 6, 2.0
    lam = torch.full((1, k), a, dtype=dtype, device=DEV)
    U = torch.eye(k, dtype=dtype, device=DEV)[None].contiguous()
    fl, dfl = torch.sqrt(lam), 0.5 / torch.sqrt(lam)
    dc = rand((1, k), 3, dtype).to(DEV)
    scale = torch.ones(1, dtype=dtype, device=DEV)
    dalpha, dbeta, dscale = raw_coeffs_bwd(lam, U, fl, dfl, dc, scale)
    torch.cuda.synchronize()
    fp = float(dfl[0, 0])
    want_alpha = torch.zeros(1, k, dtype=dtype)
    want_alpha[0, 0] = fp * float(dc[0, 0])
    want_beta = torch.zeros(1, k - 1, dtype=dtype)
    want_beta[0, 0] = fp * float(dc[0, 1])
    assert bool(torch.isfinite(dalpha).all() and torch.isfinite(dbeta).all() and torch.isfinite(dscale).all())
    assert relerr(dalpha, want_alpha) <= 4 * torch.finfo(dtype).eps
    assert relerr(dbeta, want_beta) <= 4 * torch.finfo(dtype).eps
    assert bool((dbeta[0, 1:] == 0).all()) and bool((dalpha[0, 1:] == 0).all())


def test_coeffs_vjp_on_a_nearly_degenerate_pair():
    """gap 1e-9 in fp64: above the equality threshold, so the divided difference itself is formed -- against the same formula with the same rule"""
    k = 5
    g = torch.Generator().manual_seed(9)
    U = torch.linalg.qr(torch.randn(k, k, generator=g, dtype=F64))[0][None]
    lam = torch.tensor([[1.0, 1.0 + 1e-9, 2.0, 3.0, 4.0]], dtype=F64)
    fl, dfl = torch.log(lam), 1.0 / lam
    dc, scale = torch.randn(1, k, generator=g, dtype=F64), torch.tensor([1.3], dtype=F64)
    ref = _coeffs_reference(lam, U, fl, dfl, dc, scale, rel_tol=1e-13)
    dalpha, dbeta, dscale = raw_coeffs_bwd(*(t.to(DEV).contiguous() for t in (lam, U, fl, dfl, dc, scale)))
    torch.cuda.synchronize()
    for what, got, want in (("dalpha", dalpha, ref[1]), ("dbeta", dbeta, ref[2]), ("dscale", dscale, ref[3])):
        err = relerr(got, want)
        print(f"near-degenerate {what}: {err:.2e}")
        assert err <= VALUE_TOL[F64], (what, err)


# ---------------------------------------------------------------------------------------------------------------------------
# mfx_basis_combine / _bwd
# ---------------------------------------------------------------------------------------------------------------------------
# NS: every one odd, so these run the scalar-load instantiations (VEC = 1), and with p <= 3 they stay below 16 slice workgroups: one-wave
# workgroups, 512-element slices, one slice .. nine, ragged ends.  The 16-byte loads, the 256-thread workgroups and both of their slicings
# are GEOMETRY below.
NS = [1, 7, 511, 513, 2047, 2049, 4099]
KS = [1, 2, 17, 33]  # across the 16-row buffers of sweep_rows
# (n, p) -> what the launch helpers choose, with s = ceil(n / 2048) p slice workgroups of the coarse slicing:
#   16 <= s < 128, n % (16 bytes) == 0: 256 threads, Ctx::fine -- one 16-byte load per thread and row, 512 (fp64) / 1024 (fp32) elements per slice
#   s >= 128: 256 threads, 2048-element slices, 16-byte loads;  an odd n of that size: the same with scalar loads
GEOMETRY = [(65536, 1), (32768, 3), (32772, 3), (262144, 1), (262145, 1)]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("p", [1, 3])
def test_combine_and_its_vjp_against_einsum(p, dtype):
    tol = VALUE_TOL[dtype]
    worst = 0.0
    for n in NS:
        for k in KS:
            worst = max(worst, _combine_case(n, k, p, dtype, tol))
    print(f"p={p} {dtype}: worst relative error {worst:.2e}")


def _combine_case(n, k, p, dtype, tol):
    """forward, backward, each half alone and a second run at one shape -> the worst relative error against fp64 einsum"""
    Qh, ch, dyh = rand((p, k, n), n + k, dtype), rand((p, k), n + k + 1, dtype), rand((p, n), n + k + 2, dtype)
    Q, c, dy = Qh.to(DEV), ch.to(DEV), dyh.to(DEV)
    y = raw_combine(Q, c)
    dQ, dc, _ = raw_combine_bwd(Q, c, dy)
    dQ_only, none_c, _ = raw_combine_bwd(Q, c, dy, want_c=False)
    none_q, dc_only, _ = raw_combine_bwd(Q, c, dy, want_q=False)
    y2 = raw_combine(Q, c)
    dQ2, dc2, _ = raw_combine_bwd(Q, c, dy)
    torch.cuda.synchronize()
    errs = (relerr(y, torch.einsum("pk,pkn->pn", ch.to(F64), Qh.to(F64))),
            relerr(dQ, torch.einsum("pk,pn->pkn", ch.to(F64), dyh.to(F64))),
            relerr(dc, torch.einsum("pkn,pn->pk", Qh.to(F64), dyh.to(F64))))
    assert max(errs) <= tol, (n, k, p, errs)
    assert none_c is None and none_q is None
    assert torch.equal(dQ_only, dQ) and torch.equal(dc_only, dc), (n, k, p, "a skipped half changed the other output")
    assert torch.equal(y2, y) and torch.equal(dQ2, dQ) and torch.equal(dc2, dc), (n, k, p, "two runs differ")
    return max(errs)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,p", GEOMETRY, ids=[f"n{n}-p{p}" for n, p in GEOMETRY])
def test_combine_and_its_vjp_on_the_production_geometry(n, p, dtype):
    worst = max(_combine_case(n, k, p, dtype, VALUE_TOL[dtype]) for k in (2, 33))
    print(f"n={n} p={p} {dtype}: worst relative error {worst:.2e}")


@pytest.mark.parametrize("n,k,p,dtype", [(4099, 17, 3, F32), (513, 33, 1, F64), (65536, 17, 1, F64), (32768, 5, 3, F32), (262144, 5, 1, F32)],
                         ids=["n4099-f32", "n513-f64", "fine-n65536-f64", "fine-n32768-f32", "coarse-n262144-f32"])
def test_combine_bwd_keeps_the_workspace_contract(n, k, p, dtype):
    """exactly the queried bytes between two poisoned guard bands: nothing written outside, nothing read that was not written (the results
    do not depend on the poison), and one byte less is refused before anything is written"""
    Q, c, dy = rand((p, k, n), 1, dtype).to(DEV), rand((p, k), 2, dtype).to(DEV), rand((p, n), 3, dtype).to(DEV)
    need = combine_ws_bytes(Q)
    guard = GuardedWs()
    results = []
    for poison in (0x00, 0xFF):
        guard.poison = poison
        ws = guard.take(need, DEV, label="mfx_basis_combine_bwd")
        assert ws.numel() == need
        dQ, dc, _ = raw_combine_bwd(Q, c, dy, ws=ws)
        guard.verify()
        assert bool(torch.isfinite(dQ).all() and torch.isfinite(dc).all())
        results.append((dQ.cpu(), dc.cpu()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    ref_q, ref_c, _ = raw_combine_bwd(Q, c, dy)
    assert torch.equal(ref_q.cpu(), results[0][0]) and torch.equal(ref_c.cpu(), results[0][1])
    guard.poison = 0x5A
    ws = guard.take(need, DEV, label="short")
    dQ, dc, rc = raw_combine_bwd(Q, c, dy, ws=ws, ws_bytes=need - 1, check=False)
    torch.cuda.synchronize()
    assert rc == MFX_ERR_WORKSPACE and "workspace" in _lib.get().mfx_last_error().decode()
    assert bool((dQ == -77.0).all() and (dc == -77.0).all() and (ws == 0x5A).all()), "a refused call wrote something"
    guard.verify()


def test_funm_backward_takes_exactly_the_queried_workspace(monkeypatch):
    """the Python layer under the guarded allocator: _FunmFn.backward asks for the queried size and stays inside it"""
    guard = GuardedWs(poison=0xFF, busy=_lib._ws_busy)
    monkeypatch.setattr(_lib, "_take", guard.take)
    n, k = 300, 5
    A = _spd_matrix(n, 0.5, 4.0, 2).to(DEV).requires_grad_(True)
    v = rand((2, n), 4).to(DEV).requires_grad_(True)
    y = lanczos.funm_spd(torch.sqrt, k, DenseOp())(v, A)
    gA, gv = torch.autograd.grad((y * y).sum(), (A, v))
    guard.verify()
    assert guard.handed_out >= 1 and bool(torch.isfinite(gA).all() and torch.isfinite(gv).all())


# ---------------------------------------------------------------------------------------------------------------------------
# end to end, fp64
# ---------------------------------------------------------------------------------------------------------------------------
def _spd_matrix(n, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    X, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=F64))
    lam = torch.logspace(math.log10(lo), math.log10(hi), n, dtype=F64)
    A = (X * lam) @ X.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("name", sorted(MATFUNS))
def test_funm_at_full_depth_equals_the_dense_matrix_function(name):
    n = 12
    A = _spd_matrix(n, 0.1, 10.0, 3)
    lam, X = torch.linalg.eigh(A)
    v = rand((n,), 5)
    dense = X @ (MATFUNS[name](lam) * (X.T @ v))
    got = lanczos.funm_spd(MATFUNS[name], n, DenseOp())(v.to(DEV), A.to(DEV))
    assert got.shape == (n,)
    err = relerr(got, dense)
    print(f"{name}: {err:.2e}")
    assert err <= VALUE_TOL[F64]


def test_funm_truncated_against_the_restatement():
    """n = 257, k = 24, p = 3: the restatement runs the same truncated recurrence, so the truncation error cancels and what is left is
    rounding, amplified by the sensitivity of the Krylov recurrence.  That sensitivity is measured here: the restatement's own response to a
    relative perturbation of A of 1e-16 (below one rounding of its entries); the bar is 1e-10 or 100 times that response."""
    n, k, p = 257, 24, 3
    A = _spd_matrix(n, 0.1, 10.0, 7)
    V = rand((p, n), 8)
    ref = rs.funm_batched(A, V, k, torch.sqrt)
    E = rand((n, n), 9)
    moved = rs.funm_batched(A * (1.0 + 1e-16 * 0.5 * (E + E.T)), V, k, torch.sqrt)
    response = relerr(moved, ref)
    tol = max(VALUE_TOL[F64], 100.0 * response)
    got = lanczos.funm_spd(torch.sqrt, k, DenseOp())(V.to(DEV), A.to(DEV))
    err = relerr(got, ref)
    print(f"response of the restatement to a 1e-16 perturbation {response:.2e} -> tolerance {tol:.2e}; device against restatement {err:.2e}")
    assert err <= tol


def test_funm_three_term_recurrence_against_the_restatement():
    n, k = 64, 6
    A = _spd_matrix(n, 0.5, 4.0, 11)
    V = rand((2, n), 12)
    ref = rs.funm_batched(A, V, k, torch.log, reortho="none")
    got = lanczos.funm_spd(torch.log, k, DenseOp(), reortho="none")(V.to(DEV), A.to(DEV))
    err = relerr(got, ref)
    print(f"reortho=none: {err:.2e}")
    assert err <= VALUE_TOL[F64]


def _laplacian_coo(m):
    """symmetric Dirichlet 5-point Laplacian on an m x m grid: -4 on the diagonal, 1 towards each neighbour inside the grid"""
    rows, cols, vals = [], [], []
    for i in range(m):
        for j in range(m):
            r = i * m + j
            rows.append(r), cols.append(r), vals.append(-4.0)
            for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= i + di < m and 0 <= j + dj < m:
                    rows.append(r), cols.append((i + di) * m + j + dj), vals.append(1.0)
    return torch.tensor(rows), torch.tensor(cols), torch.tensor(vals, dtype=F64)


def test_expm_lanczos_on_a_csr_laplacian_against_matrix_exp():
    m = 9
    n = m * m
    row, col, vals = _laplacian_coo(m)
    op, dvals, _ = CsrOp.from_coo(row, col, vals, n, DEV)
    dense = torch.zeros(n, n, dtype=F64).index_put((row, col), vals)
    y0 = rand((n,), 13)
    dt = 0.1
    out, info = pde_util.expm_lanczos(20)(op, dt, y0.to(DEV), dvals)
    ref = torch.linalg.matrix_exp(dt * dense) @ y0
    err = relerr(out, ref)
    print(f"expm_lanczos(20) against matrix_exp: {err:.2e}")
    assert info == {"num_matvecs": 20} and err <= VALUE_TOL[F64]


# ---------------------------------------------------------------------------------------------------------------------------
# gradients, fp64, against autograd through the restatement: n = 64, k = 6, p = 2 (well separated Ritz values)
# ---------------------------------------------------------------------------------------------------------------------------
GN, GK, GP = 64, 6, 2


def _check_grads(names, got, ref):
    for name, g, r in zip(names, got, ref):
        err = relerr(g, r)
        print(f"  d/d{name}: {err:.2e}")
        assert err <= GRAD_TOL, (name, err)


def test_gradients_dense_operator():
    A = _spd_matrix(GN, 0.5, 4.0, 21)
    V, W = rand((GP, GN), 22), rand((GP, GN), 23)
    Ac, Vc = A.clone().requires_grad_(True), V.clone().requires_grad_(True)
    ref = torch.autograd.grad((rs.funm_batched(Ac, Vc, GK, torch.sqrt) * W).sum(), (Ac, Vc))
    Ad, Vd = A.to(DEV).requires_grad_(True), V.to(DEV).requires_grad_(True)
    y = lanczos.funm_spd(torch.sqrt, GK, DenseOp())(Vd, Ad)
    got = torch.autograd.grad((y * W.to(DEV)).sum(), (Ad, Vd))
    _check_grads(("A", "v"), got, ref)


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "scalar"])
@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_gradients_gram_operator(kernel, ard):
    d = 3
    X = rand((GN, d), 31)
    raw = [torch.full((d,) if ard else (), inv_softplus(1.2), dtype=F64) + (0.1 * rand((d,), 32) if ard else 0.0),
           torch.tensor(inv_softplus(0.9), dtype=F64), torch.tensor(inv_softplus(0.5), dtype=F64)]
    V, W = rand((GP, GN), 33), rand((GP, GN), 34)
    cpu = [t.clone().requires_grad_(True) for t in (*raw, X, V)]
    K = rs.gram_matrix(cpu[3], cpu[0], cpu[1], cpu[2], kernel=kernel)
    ref = torch.autograd.grad((rs.funm_batched(K, cpu[4], GK, torch.sqrt) * W).sum(), cpu)
    dev = [t.to(DEV).requires_grad_(True) for t in (*raw, X, V)]
    apply = gp_util.gram_funm(torch.sqrt, GK, kernel=kernel)
    y = apply(dev[3], dev[4], raw_lengthscale=dev[0], raw_outputscale=dev[1], raw_noise=dev[2])
    got = torch.autograd.grad((y * W.to(DEV)).sum(), dev)
    _check_grads(("lengthscale", "outputscale", "noise", "X", "v"), got, ref)


def test_gradients_expm_lanczos_csr():
    m = 8
    row, col, vals = _laplacian_coo(m)
    op, dvals, order = CsrOp.from_coo(row, col, vals, GN, DEV)
    Y0, W = rand((GP, GN), 41), rand((GP, GN), 42)
    vc, dtc = vals.clone().requires_grad_(True), torch.tensor(0.1, dtype=F64, requires_grad=True)
    dense = torch.zeros(GN, GN, dtype=F64).index_put((row, col), vc)
    ref = torch.autograd.grad((rs.funm_batched(dense, Y0, GK, lambda lam: torch.exp(dtc * lam)) * W).sum(), (dtc, vc))
    vd, dtd = dvals.clone().requires_grad_(True), torch.tensor(0.1, dtype=F64, device=DEV, requires_grad=True)
    out, _ = pde_util.expm_lanczos(GK)(op, dtd, Y0.to(DEV), vd)
    got = torch.autograd.grad((out * W.to(DEV)).sum(), (dtd, vd))
    _check_grads(("dt", "values"), got, (ref[0], ref[1][order]))


def test_gradcheck_of_the_funm_function_alone():
    k, n = 5, 9
    Q = rand((1, k, n), 51).to(DEV).requires_grad_(True)
    diag = (2.0 + rand((1, k), 52).abs()).to(DEV).requires_grad_(True)
    off = (0.2 * rand((1, k - 1), 53)).to(DEV).requires_grad_(True)
    scale = torch.tensor([1.4], dtype=F64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda *a: lanczos._funm_apply(torch.sqrt, *a), (Q, diag, off, scale))


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 against the fp64 device path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gram_sqrt_fp64():
    return _gram_sqrt(F64, "fp32")


def _gram_sqrt(dtype, precision):
    n, d, p = 300, 4, 5
    X = rand((n, d), 61, dtype).to(DEV)
    V, W = rand((p, n), 62, dtype).to(DEV), rand((p, n), 63, dtype).to(DEV)
    raw = [torch.tensor(inv_softplus(v), dtype=dtype, device=DEV, requires_grad=True) for v in (1.0, 1.0, 0.5)]
    y = gp_util.gram_funm(torch.sqrt, 16, precision=precision)(X, V, raw_lengthscale=raw[0], raw_outputscale=raw[1], raw_noise=raw[2])
    grads = torch.autograd.grad((y * W).sum(), raw)
    return y.detach(), [g.detach() for g in grads]


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_fp32_prior_draws_against_the_fp64_device_path(precision, gram_sqrt_fp64):
    y, grads = _gram_sqrt(F32, precision)
    ev = relerr(y, gram_sqrt_fp64[0])
    egs = [relerr(g, r) for g, r in zip(grads, gram_sqrt_fp64[1])]  # three scalars, each against its own size
    print(f"{precision}: value {ev:.2e}, d/d(raw lengthscale, raw outputscale, raw noise) " + ", ".join(f"{e:.2e}" for e in egs))
    assert ev <= VALUE_TOL[F32] and max(egs) <= VALUE_TOL[F32], (ev, egs)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_shapes():
    A = _spd_matrix(8, 0.5, 4.0, 71).to(DEV)
    v = rand((8,), 72).to(DEV)
    sharded = RowShardedOp(DenseOp(), None, exchange=False)  # no communicator: any collective or launch would fail on it
    with pytest.raises(NotImplementedError, match="row-sharded"):
        lanczos.funm_spd(torch.sqrt, 3, sharded)(v, A)
    with pytest.raises(ValueError, match="depth"):
        lanczos.funm_spd(torch.sqrt, 9, DenseOp())(v, A)
    with pytest.raises(ValueError, match="depth"):
        lanczos.funm_spd(torch.sqrt, 9, DenseOp(), reortho="none")(v, A)
    one = lanczos.funm_spd(torch.sqrt, 3, DenseOp())(v, A)
    two = lanczos.funm_spd(torch.sqrt, 3, DenseOp())(v[None], A)
    assert one.shape == (8,) and two.shape == (1, 8) and torch.equal(one, two[0])
