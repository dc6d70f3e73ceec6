"""mfx_gram_block / RbfGramOp.gram_block: a dense block K(xa, xb) of the kernel matrix written to memory.

The reference is a torch-fp64 evaluation of the Gram operator's own formulas: inputs over the lengthscale, |a|^2 + |b|^2 - 2 a.b
clamped at 0, eps of the COMPUTE dtype inside Matern's square roots, and -- in the symmetric block -- the distance of a point to
itself exactly 0.

Tolerances (errors are absolute, against the outputscale s: 0 <= k <= s):
  fp64: 1e-12 s.
  fp32: the existing way to such a block is mfx_gram_cross_apply_t against the identity (what posterior_variance runs).  Its error
        against the same fp64 reference is measured at the same inputs; the new block may err at most twice that, floored at
        8 eps(fp32) s -- two correct orderings of a d-term dot product differ by that much.
Gradients are compared as tests/test_gpu_posterior_grad.py compares the cross VJP of the same dtype: |g - ref| against the sum of
the absolute values of the reference's own terms, 1e-9 in fp64 and 1e-3 in fp32."""

import ctypes as C
import math

import pytest
import torch

from matfree_extensions import _lib
from matfree_extensions.operators import RbfGramOp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = float(torch.finfo(torch.float32).eps)
GRAD_TOL = {torch.float64: 1e-9, torch.float32: 1e-3}  # tests/test_gpu_posterior_grad.py: TOL
KERNELS = ("rbf", "matern12", "matern32", "matern52")
SENTINEL = -77.0


def inv_softplus(v):
    return math.log(math.expm1(v))


def kfun(dist, kind, eps):
    if kind == "rbf":
        return torch.exp(-dist / 2)
    if kind == "matern12":
        return torch.exp(-torch.sqrt(dist + eps))
    r = torch.sqrt((3.0 if kind == "matern32" else 5.0) * dist + eps)
    if kind == "matern32":
        return (1 + r) * torch.exp(-r)
    return (1 + r + r * r / 3) * torch.exp(-r)


def ref_block(xa, xb, ls, s, kind, eps, symmetric=False):
    """s kappa(max(0, |a / l|^2 + |b / l|^2 - 2 (a / l).(b / l))) in fp64; symmetric: the diagonal at distance exactly 0"""
    a, b = xa / ls, xb / ls
    dist = ((a * a).sum(-1)[:, None] + (b * b).sum(-1)[None, :] - 2.0 * a @ b.T).clamp_min(0.0)
    if symmetric:
        dist = dist * (1.0 - torch.eye(xa.shape[0], dtype=dist.dtype, device=dist.device))
    return s * kfun(dist, kind, eps)


def raw_params(d, ard, dtype):
    ls = [inv_softplus(0.7 + 0.15 * (c % 7)) for c in range(d)] if ard else inv_softplus(1.1)
    return (torch.tensor(ls, dtype=dtype, device=DEV), torch.tensor(inv_softplus(0.8), dtype=dtype, device=DEV),
            torch.tensor(inv_softplus(0.5), dtype=dtype, device=DEV))


def points(m, d, seed):
    """fp32-representable points, so that both dtypes and the fp64 reference see the same inputs"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(m, d, device=DEV, generator=g, dtype=torch.float32).double()


def raw_block(op, cparams, xa, xb, ldo=None):
    """mfx_gram_block through ctypes into a sentinel-filled (ma, ldo) buffer"""
    lib = _lib.get()
    ma, mb = xa.shape[0], (xa if xb is None else xb).shape[0]
    ldo = mb if ldo is None else ldo
    desc = op.descriptor(cparams, xa.dtype, op.n)
    out = torch.full((ma, ldo), SENTINEL, dtype=xa.dtype, device=DEV)
    ws = _lib.scratch(int(lib.mfx_gram_block_workspace_bytes(C.byref(desc), ma, mb)), DEV)
    _lib.check(lib.mfx_gram_block(C.byref(desc), _lib.ptr(xa), ma, _lib.ptr(xb), mb, _lib.ptr(out), ldo, _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return out


def identity_block(xa, xb, kind, raw):
    """K(xa, xb) the existing way: mfx_gram_cross_apply_t of the operator over xb against the ma x ma identity (its rows come out as
    K(xb, xa) u_a = K(xa_a, xb))"""
    op = RbfGramOp(xb.contiguous(), kernel=kind)
    cparams = op.constrain(*raw)
    lib = _lib.get()
    ma, mb = xa.shape[0], xb.shape[0]
    desc = op.descriptor(cparams, xa.dtype, mb)
    eye = torch.eye(ma, dtype=xa.dtype, device=DEV)
    out = torch.empty((ma, mb), dtype=xa.dtype, device=DEV)
    ws = _lib.scratch(int(lib.mfx_gram_cross_workspace_bytes(C.byref(desc), ma)), DEV)
    _lib.check(lib.mfx_gram_cross_apply_t(C.byref(desc), _lib.ptr(xa), ma, _lib.ptr(eye), ma, _lib.ptr(out), mb, ma, _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return out


SHAPES = [(1, 1), (63, 65), (64, 64), (65, 257), (300, 37)]
DIMS = [(1, False), (3, False), (8, False), (9, True), (16, True), (20, False), (40, True)]  # register path (4, 4, 8, 12, 16), padded 32, wide (64)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", KERNELS)
@pytest.mark.parametrize("d,ard", DIMS)
def test_block_matches_the_fp64_formulas(kind, dtype, d, ard):
    raw = raw_params(d, ard, dtype)
    sp = torch.nn.functional.softplus
    ls64, s64 = sp(raw[0].double()), sp(raw[1].double())
    s = float(s64)
    eps = float(torch.finfo(dtype).eps)
    for i, (ma, mb) in enumerate(SHAPES):
        xa64, xb64 = points(ma, d, 100 + i), points(mb, d, 200 + i)
        xa, xb = xa64.to(dtype), xb64.to(dtype)
        op = RbfGramOp(xb, kernel=kind)  # (the block uses the operator's kernel, dtype and d only)
        cparams = op.constrain(*raw)
        ldo = mb + (0, 3, 64, 1, 5)[i]
        out = raw_block(op, cparams, xa, xb, ldo=ldo)
        want = ref_block(xa64, xb64, ls64, s64, kind, eps)
        err = float((out[:, :mb].double() - want).abs().max())
        if dtype == torch.float64:
            bound = 1e-12 * s
        else:
            old = float((identity_block(xa, xb, kind, raw).double() - want).abs().max())
            bound = max(2.0 * old, 8.0 * EPS32 * s)
        print(f"{kind} {dtype} d={d} ({ma}, {mb}): err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (ma, mb, err, bound)
        assert bool((out[:, mb:] == SENTINEL).all()), (ma, mb)  # the padding of every row is left alone
        assert torch.equal(op.gram_block(xa, xb, *raw), out[:, :mb])  # the Python method is the same call


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", KERNELS)
@pytest.mark.parametrize("d,ard", [(3, True), (20, True), (40, False)])
def test_symmetric_block_is_bitwise_symmetric_with_an_exact_diagonal(kind, dtype, d, ard):
    m = 130  # three tiles a side, the last one partial
    raw = raw_params(d, ard, dtype)
    xa64 = points(m, d, 7)
    xa64[5] = xa64[99]  # duplicated points, in different tiles and inside one
    xa64[70] = xa64[71]
    xa = xa64.to(dtype)
    op = RbfGramOp(xa, kernel=kind)
    cparams = op.constrain(*raw)
    out = raw_block(op, cparams, xa, None, ldo=m + 2)
    K = out[:, :m]
    assert bool((out[:, m:] == SENTINEL).all())
    assert torch.equal(K, K.T)
    # the diagonal is s kappa(0) with the distance exactly 0: every entry the same number (no round-off of the expansion, which
    # differs from point to point), which is s itself for RBF and s kappa(0) to the rounding of one exp and two products otherwise
    diag = K.diagonal()
    assert bool((diag == diag[0]).all())
    s = cparams[1]
    eps = float(torch.finfo(dtype).eps)
    if kind == "rbf":
        assert torch.equal(diag[0], s[0])
    k0 = float(kfun(torch.zeros((), dtype=torch.float64), kind, eps))
    assert abs(float(diag[0]) - float(s) * k0) <= 4 * eps * float(s)
    assert torch.equal(raw_block(op, cparams, xa[:1].contiguous(), None)[0, 0], diag[0])
    sp = torch.nn.functional.softplus
    want = ref_block(xa64, xa64, sp(raw[0].double()), sp(raw[1].double()), kind, eps, symmetric=True)
    err = (K.double() - want).abs()
    dup = torch.zeros_like(want, dtype=torch.bool)
    for i, j in ((5, 99), (70, 71)):
        dup[i, j] = dup[j, i] = True
    if dtype == torch.float64:
        bound = 1e-12 * float(s)
    else:  # the existing path at the same inputs, off the diagonal (it takes its diagonal from the expansion)
        off = ~dup & ~torch.eye(m, dtype=torch.bool, device=DEV)
        old = float((identity_block(xa, xa, kind, raw).double() - want).abs()[off].max())
        bound = max(2.0 * old, 8.0 * EPS32 * float(s))
    assert float(err[~dup].max()) <= bound, (float(err[~dup].max()), bound)
    for i, j in ((5, 99), (70, 71)):
        assert err[i, j] <= duplicate_bound(xa64[i], d, eps) * float(s), (i, j, float(err[i, j]))
    assert torch.isfinite(K).all()
    assert torch.equal(op.gram_block(xa, None, *raw), K)


def duplicate_bound(x, d, eps):
    """|kappa(0) - kappa(dist)| / s for an exactly duplicated pair off the diagonal, which keeps the clamped expansion
    |a|^2 + |a|^2 - 2 a.a: each of the three d-term sums rounds to (d + 2) eps |a / l|^2 at most (l >= 0.7 here), so dist <=
    4 (d + 2) eps |a / l|^2 =: delta, and Matern-1/2, the steepest family at 0, moves by 1 - exp(sqrt(eps) - sqrt(delta + eps)) <=
    sqrt(delta) (the others by <= 5 delta / 2)"""
    return math.sqrt(4 * (d + 2) * eps * float((x / 0.7).pow(2).sum()))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", KERNELS)
def test_cross_set_duplicates_take_the_clamped_distance(kind, dtype):
    d, ma, mb = 9, 70, 131
    raw = raw_params(d, True, dtype)
    xa64, xb64 = points(ma, d, 3) * 30.0, points(mb, d, 4) * 30.0  # large norms: the expansion's round-off is at its largest
    xa64[0], xa64[69] = xb64[130], xb64[64]  # a row of xb copied into xa, in the first and in a partial tile
    xa, xb = xa64.to(dtype), xb64.to(dtype)
    op = RbfGramOp(xb, kernel=kind)
    K = op.gram_block(xa, xb, *raw)
    assert torch.isfinite(K).all()
    s = float(op.constrain(*raw)[1])
    eps = float(torch.finfo(dtype).eps)
    k0 = float(kfun(torch.zeros((), dtype=torch.float64), kind, eps))
    assert float(K.max()) <= s * k0 * (1 + 4 * eps)  # clamped: never beyond the value at distance 0
    for a, b in ((0, 130), (69, 64)):
        assert abs(s * k0 - float(K[a, b])) <= duplicate_bound(xa64[a], d, eps) * s, (a, b, float(K[a, b]))


def test_index_arithmetic_is_64_bit():
    """rows whose a * ldo lies beyond 2^31 elements (the buffer is allocated, only its five short rows are written)"""
    d, ma, mb, ldo = 3, 5, 70, (1 << 29) + 3
    raw = raw_params(d, False, torch.float32)
    xa, xb = points(ma, d, 11).float(), points(mb, d, 12).float()
    op = RbfGramOp(xb, kernel="matern32")
    cparams = op.constrain(*raw)
    lib = _lib.get()
    desc = op.descriptor(cparams, torch.float32, op.n)
    buf = torch.empty((ma - 1) * ldo + mb + 2, dtype=torch.float32, device=DEV)
    pads = torch.as_strided(buf, (ma, 2), (ldo, 1), mb)  # the two entries behind every row
    pads.fill_(SENTINEL)
    ws = _lib.scratch(int(lib.mfx_gram_block_workspace_bytes(C.byref(desc), ma, mb)), DEV)
    _lib.check(lib.mfx_gram_block(C.byref(desc), _lib.ptr(xa), ma, _lib.ptr(xb), mb, _lib.ptr(buf), ldo, _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    got = torch.as_strided(buf, (ma, mb), (ldo, 1))
    assert torch.equal(got, op.gram_block(xa, xb, *raw))
    assert bool((pads == SENTINEL).all())
    del buf, pads, got
    torch.cuda.empty_cache()


def ref_block_grad(xa, xb, ls, s, kind, eps):
    """the block for differentiation: as ref_block, exactly duplicated pairs (the diagonal of a symmetric block among them) at
    distance 0 and held constant, as tests/test_gpu_posterior_grad.py holds them"""
    a, b = xa / ls, xb / ls
    dist = ((a * a).sum(-1)[:, None] + (b * b).sum(-1)[None, :] - 2.0 * a @ b.T).clamp_min(0.0)
    same = (xa[:, None, :] == xb[None, :, :]).all(-1)
    k = kfun(torch.where(same, torch.zeros_like(dist), dist), kind, eps)
    return s * torch.where(same, k.detach(), k)


def term_sums(xa, xb, ls, s, kind, S, eps):
    """sums of the absolute values of the terms of every gradient element: (xa, xb, lengthscale per dimension, outputscale) -- the
    scale a correctly rounded sum errs against (tests/test_gpu_posterior_grad.py: term_sums)"""
    with torch.no_grad():
        a, b = xa / ls, xb / ls
        diff = a[:, None, :] - b[None, :, :]
        dist = (diff * diff).sum(-1)
        k = kfun(dist, kind, eps)
        if kind == "rbf":
            wl = k
        elif kind == "matern12":
            r = torch.sqrt(dist + eps)
            wl = torch.where(dist > 0, torch.exp(-r) / r, torch.zeros_like(r))
        elif kind == "matern32":
            wl = 3 * torch.exp(-torch.sqrt(3 * dist + eps))
        else:
            r = torch.sqrt(5 * dist + eps)
            wl = 5.0 / 3.0 * (1 + r) * torch.exp(-r)
        lsv = ls.expand(xa.shape[1])
        W = S.abs() * wl
        mag = a.abs()[:, None, :] + b.abs()[None, :, :]
        t_xa = (W[:, :, None] * mag).sum(1) * s / lsv
        t_xb = (W[:, :, None] * mag).sum(0) * s / lsv
        t_ls = (W[:, :, None] * diff * diff).sum((0, 1)) * s / lsv
        t_s = (S.abs() * k).sum()
        return t_xa, t_xb, t_ls, t_s


def check(got, want, scale, tol, what):
    err = (got.double() - want).abs() / (scale + 1e-300)
    print(f"  {what}: {float(err.max()):.3e} (tol {tol:.0e})")
    assert float(err.max()) <= tol, (what, float(err.max()))


def grad_params(d, ard):
    return tuple(r.double().requires_grad_(True) for r in raw_params(d, ard, torch.float64))


# (kernel, d, ard, ma, mb): every kernel, the register sweeps (padded 4, 12, 32) and the wide one, sizes off the tile
GRAD_CASES = [("rbf", 3, True, 70, 131), ("matern12", 9, True, 33, 65), ("matern32", 20, False, 65, 70), ("matern52", 40, True, 37, 64),
              ("matern52", 1, False, 64, 64)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,d,ard,ma,mb", GRAD_CASES)
def test_gradients_match_autograd_on_the_fp64_formulas(kind, d, ard, ma, mb, dtype):
    xa0, xb0 = points(ma, d, 21), points(mb, d, 22)
    if d > 1:  # (on a line fp32 Matern weights near a duplicate are not comparable: tests/test_gpu_posterior_var.py, CASES)
        xa0[0] = xb0[3]
    S = points(ma, mb, 23)
    raw = grad_params(d, ard)
    xa, xb = xa0.clone().requires_grad_(True), xb0.clone().requires_grad_(True)
    op = RbfGramOp(points(4, d, 24).to(dtype), kernel=kind)  # its own X plays no part
    K = op.gram_block(xa, xb, *raw)
    assert K.shape == (ma, mb) and K.dtype == dtype
    gxa, gxb, gl, gs, gn = torch.autograd.grad((S.to(dtype) * K).sum(), (xa, xb, *raw), allow_unused=True)
    assert gn is None  # no noise term in a block

    eps = float(torch.finfo(dtype).eps)
    sp = torch.nn.functional.softplus
    ls = sp(raw[0]).detach().to(dtype).double().reshape(-1).requires_grad_(True)
    s = sp(raw[1]).detach().to(dtype).double().requires_grad_(True)
    xar, xbr = xa0.clone().requires_grad_(True), xb0.clone().requires_grad_(True)
    rxa, rxb, rl, rs = torch.autograd.grad((S * ref_block_grad(xar, xbr, ls, s, kind, eps)).sum(), (xar, xbr, ls, s))
    t_xa, t_xb, t_ls, t_s = term_sums(xa0, xb0, ls.detach(), s.detach(), kind, S, eps)
    sig_l, sig_s = torch.sigmoid(raw[0].detach()).reshape(-1), torch.sigmoid(raw[1].detach())
    tol = GRAD_TOL[dtype]
    check(gxa, rxa, t_xa, tol, "xa")
    check(gxb, rxb, t_xb, tol, "xb")
    check(gl.reshape(-1), rl * sig_l, (t_ls if ard else t_ls.sum()) * sig_l, tol, "lengthscale")
    check(gs, rs * sig_s, t_s * sig_s, tol, "outputscale")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,d,ard,m", [("rbf", 3, True, 70), ("matern12", 9, False, 65), ("matern32", 40, True, 37),
                                          ("matern52", 20, True, 130)])
def test_symmetric_gradient_is_the_sum_of_both_slots(kind, d, ard, m, dtype):
    xa0 = points(m, d, 31)
    xa0[5] = xa0[m - 1]
    S = points(m, m, 32)  # not symmetric
    raw = grad_params(d, ard)
    op = RbfGramOp(points(4, d, 33).to(dtype), kernel=kind)
    xa = xa0.clone().requires_grad_(True)
    K = op.gram_block(xa, None, *raw)
    gxa, gl, gs, gn = torch.autograd.grad((S.to(dtype) * K).sum(), (xa, *raw), allow_unused=True)
    assert gn is None

    eps = float(torch.finfo(dtype).eps)
    sp = torch.nn.functional.softplus
    ls = sp(raw[0]).detach().to(dtype).double().reshape(-1).requires_grad_(True)
    s = sp(raw[1]).detach().to(dtype).double().requires_grad_(True)
    xr = xa0.clone().requires_grad_(True)
    rxa, rl, rs = torch.autograd.grad((S * ref_block_grad(xr, xr, ls, s, kind, eps)).sum(), (xr, ls, s))
    t_xa, t_xb, t_ls, t_s = term_sums(xa0, xa0, ls.detach(), s.detach(), kind, S, eps)
    sig_l, sig_s = torch.sigmoid(raw[0].detach()).reshape(-1), torch.sigmoid(raw[1].detach())
    tol = GRAD_TOL[dtype]
    check(gxa, rxa, t_xa + t_xb, tol, "xa")
    check(gl.reshape(-1), rl * sig_l, (t_ls if ard else t_ls.sum()) * sig_l, tol, "lengthscale")
    check(gs, rs * sig_s, t_s * sig_s, tol, "outputscale")
    # the two slots of the rectangular block over the same points (its diagonal pairs add nothing to an input gradient)
    a, b = xa0.clone().requires_grad_(True), xa0.clone().requires_grad_(True)
    ga, gb = torch.autograd.grad((S.to(dtype) * op.gram_block(a, b, *raw)).sum(), (a, b))
    check(gxa, ga + gb, t_xa + t_xb, tol, "xa against both slots")


def test_a_gradient_reaches_the_operators_inputs_through_the_xb_slot():
    d, m, n = 3, 37, 70
    X = points(n, d, 41).requires_grad_(True)
    xs = points(m, d, 42)
    raw = grad_params(d, True)
    op = RbfGramOp(X, kernel="matern32")
    S = points(m, n, 43)
    (gX,) = torch.autograd.grad((S * op.gram_block(xs, op.X, *raw)).sum(), (X,))
    b = X.detach().clone().requires_grad_(True)
    (want,) = torch.autograd.grad((S * RbfGramOp(X.detach(), kernel="matern32").gram_block(xs, b, *raw)).sum(), (b,))
    assert torch.equal(gX, want)
    only_s = torch.autograd.grad(op.gram_block(xs, op.X, *raw).sum(), (raw[1],))[0]  # just one gradient asked for
    assert torch.isfinite(only_s)
